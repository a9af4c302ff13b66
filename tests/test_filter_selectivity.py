"""The filters' selectivity: `rescored_pairs` and `retry_queries` of every filter engine against the host model of
tests/selectivity_model.py (what the model restates and how its bracket is made: that module's docstring; why the assertions
below are sharp: tests/test_selectivity_model_cpu.py, conditions (a) to (e)).

Every answer of every engine is pinned bit for bit elsewhere; a band that is too small is caught by tests/test_filter_bounds.py.
A band that is too WIDE, a threshold one level late, an order statistic from the wrong grid point, a seen fraction counted from
the radices instead of the query's own range or a merge that forgets to lower tau returns identical bits and only hands more
rows to hvs_k_rescore, or sends more queries through a retry batch.  Here, per case (selectivity_model.CASES: gen-v1 rows at
n = 32768 (K = 2) and n = 70001 (K = 3, ragged last block), k = 37, sample_proportion = 0.5, queries outside the INT8 box, FP16
on PCA-like rows; 96 queries of all four types plus 16 type-3 queries of 150-400 rows), engine (INT8 plain in both operand
layouts, INT8 rotated, BF16, FP16) and regime:

* the requested engine ran, HVS_TIMING_I8_ROTATED is as asked, the answers are bit-equal to the oracle -- counts are asserted
  only after that;
* proven thresholds (HVS_GUESS_MID=256): no retry, `fallback_queries` = the model's exact list, sum lo <= rescored_pairs <= sum hi;
* guessed thresholds, at the batch's default target and at HVS_GUESS_PFAIL=1: `retry_queries` and hvs_last_reruns equal the
  model's retry set exactly (it depends on exact distances only), rescored_pairs lies in the bracket summed over the first
  pass and the retry pass;
* a build with -DHVS_MUTANT_BAND_SCALE=1.25 answers every case correctly, lands ABOVE the production bracket and inside the
  model's own bracket for that band: the production assertions would fail on a filter that is merely too generous.  FP16 is
  left out of it (the band x 1.25 moves its count by 2 bracket widths: test_conditions_of_the_gpu_cases has the numbers).

Queries on a grid edge of the guess table (model: `excluded`) are not sent.  Each context reserves room for RESERVE_NQ queries
(hvs_reserve) before its call, so that a batch of 112 gets lists of 4096 keys: under proven thresholds a type-0 query appends
up to 1920 keys at the radix-16 level, and a fresh context's 1024 would send it to a retry batch for its list's sake.

Every library and environment runs in a child process of its own (the settings are read when the library loads), one at a
time, under a time limit; after a child that died or timed out nothing more is started.

Measured against modelled (MI355X), rescored_pairs [sum lo, sum hi] and retried queries, INT8 in the 16x16x64 layout:
  case    format   proven                      default                    reckless (retried)
  v1_32k  i8      193548 [193545, 193551]     39473 [39470, 39473]        57940 [57937, 57943] (21)
  v1_32k  i8_rot  227981 [227956, 228012]     54184 [54171, 54196]        73277 [73269, 73293] (21)
  v1_32k  bf16    183801 [183748, 183858]     35638 [35620, 35658]        53918 [53896, 53940] (21)
  v1_70k  i8      207561 [207556, 207567]     41778 [41774, 41779]        49671 [49669, 49673] (15)
  v1_70k  i8_rot  262205 [262164, 262255]     60571 [60555, 60586]        68580 [68566, 68599] (15)
  v1_70k  bf16    192775 [192693, 192867]     37212 [37188, 37244]        44908 [44877, 44932] (15)
  k37     i8      78691 [78691, 78693]        -                           -
  k37     bf16    72998 [72961, 73024]        -                           -
  half    i8      323962 [323957, 323967]     75568 [75567, 75570]        71975 [71973, 71978] (9)
  half    i8_rot  370205 [370170, 370230]     99727 [99709, 99739]        92186 [92168, 92191] (9)
  half    bf16    310637 [310566, 310702]     69146 [69112, 69189]        66580 [66552, 66619] (9)
  out     i8      188871 [188868, 188873]     -                           54671 [54670, 54674] (19)
  f16     f16     182691 [182656, 182725]     34715 [34698, 34735]        48746 [48728, 48767] (18)
(the 32x32x32 layout gave the same counts in every plain INT8 case; proven and default retried none; the out case's 4 far queries
went to the exact engine in every regime)
Band x 1.25 build, measured and [sum lo, sum hi] of the model with that band:
  v1_32k  i8      198176 [198174, 198180]     41403 [41401, 41405]
  v1_32k  i8_rot  243133 [243105, 243157]     61280 [61266, 61293]
  v1_32k  bf16    185848 [185794, 185893]     36390 [36368, 36413]
  v1_70k  i8      214703 [214700, 214710]     44063 [44062, 44065]
  v1_70k  i8_rot  286977 [286922, 287021]     69950 [69930, 69965]
  v1_70k  bf16    195834 [195752, 195929]     38141 [38116, 38171]
  k37     i8      81416 [81414, 81417]        -
  k37     bf16    74225 [74180, 74264]        -
  half    i8      330344 [330339, 330350]     78852 [78849, 78853]
  half    i8_rot  390100 [390074, 390135]     110944 [110927, 110972]
  half    bf16    313516 [313433, 313584]     70431 [70390, 70459]
  out     i8      194342 [194339, 194344]     -

Caps, cursors and a row mask (selectivity_model.ATTACH over ATTACH_MATRIX; what the walk restates of each: that module's
docstring, "Attachments").  Each changes a threshold, a list's contents or a retry decision, so a mistake there -- a cap-derived
theta with a band too wide, a retry batch that starts from +inf, a final check that reads `tau == +inf`, a level whose theta
forgets the cap, keys in front of a cursor in the order statistic, tombstones that do not hold in one tile format, a tau thinned
by dead rows that retries the wrong queries -- returns identical bits.  The attachments come as .npy files and go through the
public API (Engine.set_row_mask, Engine.query(max_dist2=, after=)), padding on; one engine per (case, format) answers its cells
one call each, the cells with the mask last (it is set once and stays).  Per cell, answers first: ids and distance bits equal
to the padded answers the features' own host models give (selectivity_model.expected_answers; the key order is total, so nothing
is loosened for ties), hvs_within_info / hvs_after_info as those answers imply; then `retry_queries`, `fallback_queries` and both
re-run lists exactly, `rescored_pairs` in [sum lo, sum hi] over both passes, `dead_survivors` in the model's bracket for the dead
rows (which is one number in every cell; 0 without a mask).  The band x 1.25 build lands above the production bracket and inside
the model's for that band under cap_kth, after_p2 and mask.

Measured against modelled (MI355X), rescored_pairs [sum lo, sum hi], retried queries in parentheses, `dead` = dead_survivors
(measured = modelled):
  case    format  attachment  proven                      default                    reckless (retried)
  v1_32k  i8      cap_kth      14003 [ 14003,  14004]     14003 [14003, 14004]        16201 [16201, 16202] (21)
  v1_32k  i8      cap_mixed    49537 [ 49535,  49539]     12157 [12156, 12158]        15272 [15271, 15273] (5)
  v1_32k  i8      after_p2    204390 [204388, 204393]     51680 [51676, 51681]        76243 [76240, 76244] (22)
  v1_32k  i8      after_deep  662150 [662147, 662155]    547561 [547557, 547563]     550070 [550069, 550070] (9)
  v1_32k  i8      mask        279251 [279249, 279252]     58249 [58245, 58250]        53340 [53337, 53341] (10)
  v1_32k  i8      cap_after    52132 [ 52132,  52133]     15034 [15033, 15035]        23146 [23146, 23147] (6)
  v1_32k  i8      all          31291 [ 31291,  31293]     31190 [31190, 31192]        30819 [30818, 30823] (12)
  v1_32k  i8_rot  cap_kth      20473 [ 20466,  20478]     20473 [20466, 20478]        23782 [23775, 23787] (21)
  v1_32k  i8_rot  cap_mixed    59221 [ 59216,  59231]     17170 [17166, 17176]        20120 [20117, 20130] (5)
  v1_32k  i8_rot  after_p2    241478 [241456, 241505]     70381 [70369, 70393]        96826 [96811, 96836] (22)
  v1_32k  i8_rot  after_deep  690497 [690475, 690514]    562010 [561998, 562024]     563570 [563563, 563579] (9)
  v1_32k  i8_rot  mask        312515 [312491, 312540]     76341 [76332, 76355]        67198 [67190, 67208] (10)
  v1_32k  i8_rot  cap_after    62502 [ 62490,  62515]     21028 [21023, 21036]        29888 [29882, 29897] (6)
  v1_32k  i8_rot  all          43730 [ 43723,  43740]     43606 [43599, 43618]        43546 [43535, 43554] (12)
  v1_32k  bf16    cap_kth      12298 [ 12290,  12304]     12298 [12290, 12304]        14218 [14209, 14224] (21)
  v1_32k  bf16    cap_mixed    46781 [ 46764,  46795]     10860 [10850, 10868]        13992 [13985, 14000] (5)
  v1_32k  bf16    after_p2    193814 [193757, 193864]     46855 [46824, 46882]        70815 [70777, 70844] (22)
  v1_32k  bf16    after_deep  654060 [654015, 654120]    543727 [543711, 543743]     546506 [546491, 546529] (9)
  v1_32k  bf16    mask        269315 [269261, 269366]     53452 [53411, 53474]        49686 [49662, 49709] (10)
  v1_32k  bf16    cap_after    49139 [ 49116,  49147]     13508 [13500, 13517]        21409 [21396, 21417] (6)
  v1_32k  bf16    all          28018 [ 28001,  28036]     27935 [27919, 27952]        27615 [27597, 27629] (12)
  v1_70k  i8      cap_mixed   -                           13648 [13646, 13648]        17376 [17375, 17376] (8)
  v1_70k  i8      after_p2    -                           54554 [54552, 54555]        80078 [80076, 80084] (22)
  v1_70k  i8      mask        -                           47154 [47153, 47156]        49523 [49520, 49525] (10)
  v1_70k  i8      all         -                           32751 [32750, 32753]        33009 [33009, 33010] (15)
  half    i8      mask        -                          118391 [118388, 118394]      -
  half    i8      all         -                           59016 [59014, 59019]        -
  f16     f16     cap_kth     -                           11193 [11189, 11197]        -
  f16     f16     after_p2    -                           45212 [45191, 45237]        -
  f16     f16     mask        -                           50992 [50964, 51012]        -
(proven and default retried none, no cell sent a query to the exact engine; the 32x32x32 layout gave the 16x16x64 counts in all
seven default cells of v1_32k i8.  dead under `mask`: v1_32k 10213 / 283 / 1203 (proven / default / reckless) in all three
formats, v1_70k 296 / 200 (default / reckless), half 2435, f16 1071; 0 in every cell without a mask and under `all`, whose cap
keeps every theta finite)
Band x 1.25 build under attachments, default thresholds, measured and [sum lo, sum hi] of the model with that band:
  v1_32k  i8      cap_kth      14791 [14790, 14791]      after_p2  54133 [54128, 54137]      mask  60635 [60633, 60636]
  v1_32k  bf16    cap_kth      12668 [12660, 12681]      after_p2  47893 [47863, 47924]      mask  54460 [54434, 54485]

Exclusion lists (selectivity_model.EXCL_ATTACH; the walk's rules: that module's docstring, "Lists").  A list is tested
at every admission point and once more in the final kernel, so an admission test missing in hvs_k_rescore or in the seed, a retry
batch that runs without the lists, an order statistic drawn from lists that still hold listed keys, or a refused-keys counter that
drops a pass all return identical bits.  The lists come as a CSR in .npy files and go through Engine.query(exclude=), cut to the
queries sent.  Per cell, in this order: answers equal to selectivity_model.expected_answers (the law of tests/exclude_model.py) in
ids and distance bits, the engine and the rotation flag as asked; hvs_exclude_info -- excluding_queries = queries sent, kept_slots
and underfull_queries as those answers imply, and under ex_all the caps' and cursors' own counts; retry and exact lists exactly;
rescored_pairs in [sum lo, sum hi] and dead_survivors in its bracket; refused_keys EQUAL to the model's sum of `refused` -- in
the `out` cells, whose four far queries the exact engine answers, strictly above the filter-answered queries' sum (the re-run
sink's refused keys, counter slot 26); and the ex_p1 cell's rescored_pairs and retry list equal to those MEASURED for after_p2
in the same child on the same engine: excluding page 1 re-scores the pairs the page-2 cursor re-scores.

Measured against modelled (MI355X), rescored_pairs [sum lo, sum hi], retried queries in parentheses:
  case    format  attachment  proven                      default                    reckless (retried)
  v1_32k  i8      ex_p1       204390 [204388, 204393]     51680 [51676, 51681]        76243 [76240, 76244] (22)
  v1_32k  i8      ex_deep     229891 [229888, 229897]     79650 [79644, 79655]        87407 [87406, 87410] (12)
  v1_32k  i8      ex_scatter  224738 [224732, 224741]     65148 [65147, 65151]        77509 [77509, 77509] (18)
  v1_32k  i8      ex_all       31291 [ 31291,  31293]     31291 [31291, 31293]        31545 [31545, 31547] (1)
  v1_32k  i8_rot  ex_p1       241478 [241456, 241505]     70381 [70369, 70393]        96826 [96811, 96836] (22)
  v1_32k  i8_rot  ex_deep     272348 [272318, 272375]    105114 [105094, 105142]     112653 [112638, 112666] (12)
  v1_32k  i8_rot  ex_scatter  267140 [267114, 267170]     87402 [87384, 87409]       100364 [100355, 100379] (18)
  v1_32k  i8_rot  ex_all       43730 [ 43723,  43740]     43730 [43723, 43740]        44109 [44102, 44119] (1)
  v1_32k  bf16    ex_p1       193814 [193757, 193864]     46855 [46824, 46882]        70815 [70777, 70844] (22)
  v1_32k  bf16    ex_deep     217827 [217768, 217911]     72822 [72786, 72859]        80610 [80579, 80656] (12)
  v1_32k  bf16    ex_scatter  212964 [212908, 213027]     59207 [59166, 59235]        71354 [71323, 71388] (18)
  v1_32k  bf16    ex_all       28018 [ 28001,  28036]     28018 [28001, 28036]        28244 [28227, 28262] (1)
  v1_70k  i8      ex_p1       -                           54554 [54552, 54555]        80078 [80076, 80084] (22)
  v1_70k  i8      ex_scatter  -                           68558 [68556, 68561]        75807 [75804, 75811] (15)
  v1_70k  i8      ex_all      -                           32960 [32959, 32961]        35589 [35588, 35590] (10)
  half    i8      ex_deep     -                          149915 [149912, 149916]      -
  f16     f16     ex_p1       -                           45212 [45191, 45237]        -
  out     i8      ex_p1       199158 [199155, 199161]     -                           66680 [66677, 66682] (18)
(every ex_p1 figure is the after_p2 figure of the tables above, measured in the same child; proven and default retried none; the
32x32x32 layout gave 51680 under ex_p1 as well.  Under ex_all 85 unlisted keys or fewer lie within the cap, so at n = 32768 no
threshold ever leaves it under proven and default thresholds and one query is retried under reckless ones; n = 70001 retries 10.)
refused_keys, measured = modelled in every cell (proven / default / reckless; the same in all three formats of v1_32k):
  v1_32k  ex_p1 11200 / 11200 / 13400    ex_deep 36796 / 36796 / 40968    ex_scatter 31072 / 23105 / 21067    ex_all 8778 / 8778 / 8846
  v1_70k  ex_p1 - / 11200 / 13400        ex_scatter - / 23268 / 20104     ex_all - / 8941 / 9592
  half    ex_deep 35710 (default)        f16  ex_p1 11200 (default)
  out     ex_p1 11200 (proven) and 13000 (reckless) against 10800 and 12600 of the 108 filter-answered queries: the four far
          queries' 100 listed rows each were refused by the exact engine's re-run, and counted through the sink
Band x 1.25 build under ex_p1, default thresholds (refused_keys 11200 as in production):
  v1_32k  i8      54133 [54128, 54137]      bf16    47893 [47863, 47924]

Shared row sets (selectivity_model.RSET_ATTACH; the walk's rules: that module's docstring, "Row sets").  The tiles
carry no membership, so a set costs selectivity and nothing else: a set test missing in hvs_k_rescore but present in the seed, a
retry batch that runs without `set_of`, non-members that enter the lists and the order statistics and leave in hvs_keep_unlisted
only, a sub-pass whose refusals are not handed over, refusals booked on the list's counter instead of the set's -- all return
identical bits.  Every set of a case lies in one table (selectivity_model.case_set_table: at n = 32768 the 4 + 4 + 4 + 2 sets of
rs_half, rs_sparse, rs_ranges, rs_edges and the 112 of rs_page1), shipped as packed words in one .npy file and loaded once per
engine (Engine.set_row_sets); a cell's indices go through Engine.query(row_set=), cut to the queries sent -- under rs_list and
rs_all, where `row_set=` cannot stand beside the others in one call, through upload_queries, the attach calls and
query_resident.  Per cell, in this order: answers equal to selectivity_model.expected_answers (the law of
tests/row_sets_model.py), engine and rotation flag as asked; hvs_row_sets_info -- restricted_queries = the queries sent whose index
is not 0xFFFFFFFF, kept_slots and underfull_queries as those answers imply (all zero in a cell without sets); hvs_exclude_info all
zero without lists; retry and exact lists exactly; rescored_pairs in [sum lo, sum hi], dead_survivors in its bracket;
hvs_row_sets_info.refused_keys EQUAL to the model's sum of `set_refused`, in the `out` cells strictly above the filter-answered
queries' sum (the sink, counter slot 36), and under rs_list and rs_all hvs_exclude_info.refused_keys equal to `refused` as well;
the rs_page1 cell's rescored_pairs, retry list and refused keys equal to those MEASURED for ex_p1 in the same child on the same
engine.

Measured against modelled (MI355X), rescored_pairs [sum lo, sum hi], retried queries in parentheses:
  case    format  attachment  proven                      default                    reckless (retried)
  v1_32k  i8      rs_half     303608 [ 303602,  303610]    68469 [  68467,   68472]   117213 [ 117208,  117216] (31)
  v1_32k  i8      rs_sparse   679433 [ 679420,  679437]   265342 [ 265339,  265345]   238907 [ 238903,  238915] (17)
  v1_32k  i8      rs_ranges   474700 [ 474694,  474705]   120620 [ 120618,  120625]   125526 [ 125518,  125527] (16)
  v1_32k  i8      rs_edges    791327 [ 791324,  791328]   688287 [ 688284,  688287]   699384 [ 699382,  699385] (13)
  v1_32k  i8      rs_page1    204390 [ 204388,  204393]    51680 [  51676,   51681]    76243 [  76240,   76244] (22)
  v1_32k  i8      rs_list     332140 [ 332132,  332146]    98709 [  98707,   98711]   134045 [ 134042,  134047] (23)
  v1_32k  i8      rs_all       76609 [  76607,   76610]    73742 [  73740,   73743]    73933 [  73930,   73936] (11)
  v1_32k  i8_rot  rs_half     347160 [ 347140,  347197]    90533 [  90516,   90551]   141985 [ 141972,  142006] (31)
  v1_32k  i8_rot  rs_sparse   732929 [ 732885,  732968]   317335 [ 317295,  317356]   284768 [ 284720,  284809] (17)
  v1_32k  i8_rot  rs_ranges   521767 [ 521741,  521814]   154035 [ 154015,  154071]   154075 [ 154050,  154103] (16)
  v1_32k  i8_rot  rs_edges    814186 [ 814169,  814210]   698100 [ 698091,  698108]   709259 [ 709256,  709272] (13)
  v1_32k  i8_rot  rs_page1    241478 [ 241456,  241505]    70381 [  70369,   70393]    96826 [  96811,   96836] (22)
  v1_32k  i8_rot  rs_list     381845 [ 381812,  381881]   129400 [ 129382,  129425]   166104 [ 166083,  166124] (23)
  v1_32k  i8_rot  rs_all      102086 [ 102075,  102107]    98475 [  98465,   98495]    99147 [  99132,   99175] (11)
  v1_32k  bf16    rs_half     291067 [ 290992,  291151]    62619 [  62577,   62642]   110588 [ 110545,  110621] (31)
  v1_32k  bf16    rs_sparse   663651 [ 663556,  663731]   250585 [ 250502,  250668]   226070 [ 226001,  226144] (17)
  v1_32k  bf16    rs_ranges   460861 [ 460768,  460944]   111526 [ 111468,  111581]   117962 [ 117925,  118001] (16)
  v1_32k  bf16    rs_edges    784684 [ 784645,  784726]   685700 [ 685690,  685714]   696792 [ 696776,  696810] (13)
  v1_32k  bf16    rs_page1    193814 [ 193757,  193864]    46855 [  46824,   46882]    70815 [  70777,   70844] (22)
  v1_32k  bf16    rs_list     317827 [ 317736,  317901]    90389 [  90346,   90441]   125114 [ 125067,  125160] (23)
  v1_32k  bf16    rs_all       69761 [  69725,   69795]    67173 [  67146,   67202]    67281 [  67248,   67317] (11)
  v1_70k  i8      rs_sparse  -                            302362 [ 302343,  302369]   358702 [ 358696,  358707] (17)
  v1_70k  i8      rs_ranges  -                            129214 [ 129209,  129216]   150646 [ 150642,  150652] (15)
  v1_70k  i8      rs_edges   -                           1475759 [1475757, 1475760]  -
  v1_70k  i8      rs_all     -                             77747 [  77744,   77749]    78083 [  78077,   78088] (14)
  half    i8      rs_half    -                            126789 [ 126789,  126792]  -
  f16     f16     rs_half    -                             61620 [  61597,   61649]  -
  out     i8      rs_half     292595 [ 292591,  292598]  -                            108018 [ 108015,  108020] (28)
(every rs_page1 figure is the ex_p1 and after_p2 figure of the tables above, measured in the same child; proven and default
retried none -- the retry behaviour of sparse sets shows under `reckless`; the 32x32x32 layout gave the 16x16x64 counts in all seven
default cells of v1_32k i8.  v1_70k / rs_edges is a row of its own in the matrix: n = 32768 is a multiple of 64, and only at n = 70001
does the all-ones set have its 15 bits past n to be dirty.  rs_all takes the (8 k)-th matched distance as its cap where ex_all
takes the (3 k)-th -- selectivity_model.attachment says why.  No disagreement was met: no cell needed a rule the model lacked, and
no group's survivor entries came near `gcap` -- a run of survivors takes an eighth of its length in entries, condition (q).)
Row sets' refused_keys, measured = modelled in every cell (proven / default / reckless; the same in all three formats of v1_32k),
with hvs_exclude_info.refused_keys in parentheses where lists are attached, measured = modelled as well:
  v1_32k  rs_half  135190 / 38762 / 62910      rs_sparse 576401 / 231898 / 209817      rs_ranges 329541 / 92405 / 96304
  v1_32k  rs_edges 672311 / 672311 / 672311 (the 38 empty-set queries' ranges, once)     rs_page1 11200 / 11200 / 13400 (= ex_p1's)
  v1_32k  rs_list  132642 (31072) / 37243 (29375) / 55151 (30137)      rs_all 17003 (28352) / 16983 (27161) / 17655 (26850)
  v1_70k  rs_sparse - / 257056 / 317426    rs_ranges - / 97332 / 115355    rs_edges - / 1459871 / -    rs_all - / 19155 (27566) / 20489 (26932)
  half    rs_half  30549 (default)         f16  rs_half 39323 (default)
  out     rs_half  151082 (proven) and 80214 (reckless) against 128620 and 57752 of the 108 filter-answered queries: three of the
          four far queries carry a set, the exact engine's re-run refused their rows and counted them through the sink
Band x 1.25 build under rs_half, default thresholds (refused_keys 38762 as in production):
  v1_32k  i8      71316 [71314, 71317]      bf16    63837 [63803, 63863]
CPU figures of the set cells' conditions (tests/test_selectivity_model_cpu.py, (l) to (s)): keys asked for that are listed AND
outside the set, rs_list 12595 / 12580 / 13061; queries with fewer than k members to answer with under rs_ranges 10 of 112 at n =
32768 and 13 at n = 70001 (none with no member at all: the narrow type-3 ranges hold 150-400 rows of random ids, a quarter of them
in the set), under rs_edges 38 with none; longest list 1840 keys of 4096; at most 149894 survivor entries at one level of 524288
(v1_70k / rs_edges; rs_sparse proven 135961 in the rotated format); wrong rules against the right one at v1_32k i8: set_in_lists [39470, 39473] and set_seed_only [55182, 55187]
against [68467, 68472] (default), set_retry_dropped [88120, 88128] against [117208, 117216] (reckless), set_F_members [67952, 67957]
against [68467, 68472], set_before_list refused / set_refused 18477 / 145237 against 31072 / 132642 (rs_list, proven).
"""
import importlib
import os

import numpy as np
import pytest

import bound_model as BM
import hvs_testlib as T
import selectivity_model as SM

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
ENGINE = {BM.PLAIN_I8: (PKG.ENGINE_MFMA_I8, "0"), BM.ROT_I8: (PKG.ENGINE_MFMA_I8, "1"), BM.BF16: (PKG.ENGINE_MFMA_FILTER, None),
          BM.FP16: (PKG.ENGINE_MFMA_F16, None)}
HVS_TIMING_I8_ROTATED = 4
CHILD_TIMEOUT = 300

_CHILD = r"""
import importlib, json, os, sys, numpy as np
sys.path.insert(0, '.')
PKG = importlib.import_module('project---hybrid-vector-search-queries_amd')
spec = json.loads(sys.argv[1])
out = {}
for tag, data, engine, rot, k, sp in spec['runs']:
    z = np.load(os.path.join(spec['dir'], data + '.npz'))
    keep = np.load(os.path.join(spec['dir'], tag + '.keep.npy'))
    if rot is None:
        os.environ.pop('HVS_I8_ROTATE', None)
    else:
        os.environ['HVS_I8_ROTATE'] = rot
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(k)
        e.load_data(z['nodes'])
        e.reserve(spec['reserve'])
        ids, d = e.query(z['queries'][keep], sp)
        t = e.last_timing()
        reruns = [e.last_reruns(0).tolist(), e.last_reruns(1).tolist()]
    np.savez(os.path.join(spec['out'], tag + '.npz'), ids=ids, dists=d)
    out[tag] = dict(engine=int(t.engine), fallback=int(t.fallback_queries), retry=int(t.retry_queries), flags=int(t.flags),
                    rescored=int(t.rescored_pairs), exact_list=reruns[0], retry_list=reruns[1])
print('RESULT ' + json.dumps(out))
"""


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("selectivity")
    for case in SM.CASES:
        nodes, queries = SM.case_data(case)
        np.savez(d / (case.name + ".npz"), nodes=nodes, queries=queries)
    return d


@pytest.fixture(scope="module")
def wide_band_lib(tmp_path_factory):
    """The one extra build: the library's own source with the band x 1.25, through the existing switch."""
    return T.build_variant_libs(tmp_path_factory.mktemp("wide_band"), {"band_scale_1.25": ["-DHVS_MUTANT_BAND_SCALE=%s" % SM.MUTANT_SCALE]})["band_scale_1.25"]


_refs = {}


def _reference(case):
    """The oracle's answers of a case, computed once."""
    if case.name not in _refs:
        nodes, queries = SM.case_data(case)
        with T.oracle_k(case.k):
            _refs[case.name] = T.oracle_query(nodes, queries, case.sp)
    return _refs[case.name]


def _runs(regime, shape, mutant):
    runs = []
    for case in SM.CASES:
        if regime not in case.regimes:
            continue
        for fmt in case.fmts:
            if (shape == "32" and fmt != BM.PLAIN_I8) or (mutant and fmt == BM.FP16):
                continue
            runs.append((case, fmt))
    return runs


def _run(work_dir, regime, shape, lib=None):
    """One child: every (case, format) of the regime; returns [(case, fmt, keep, model walk, ids, dists, timing)]."""
    runs = _runs(regime, shape, lib is not None)
    label = "%s-%s-%s" % ("wide" if lib else "production", regime, shape)
    out_dir = work_dir / label
    out_dir.mkdir(exist_ok=True)
    spec_runs, keeps = [], []
    for case, fmt in runs:
        w = SM.case_walk(case, fmt, regime)            # the production model decides what is sent, for either library
        keep = np.nonzero(~w["excluded"])[0]
        tag = "%s-%s-%s" % (label, case.name, fmt)
        np.save(work_dir / (tag + ".keep.npy"), keep)
        engine, rot = ENGINE[fmt]
        spec_runs.append((tag, case.name, engine, rot, case.k, case.sp))
        keeps.append((tag, keep, w))
    env = dict(os.environ, HVS_I8_SHAPE=shape)
    for name in ("HVS_I8_ROTATE", "HVS_LIB", "HVS_GUESS_MID", "HVS_GUESS_PFAIL", "HVS_RADICES"):
        env.pop(name, None)
    env.update(SM.REGIMES[regime]["env"])
    if lib:
        env["HVS_LIB"] = lib
    timing = T.run_child(_CHILD, dict(dir=str(work_dir), out=str(out_dir), runs=spec_runs, reserve=SM.RESERVE_NQ), env, label, CHILD_TIMEOUT)
    res = []
    for (case, fmt), (tag, keep, w) in zip(runs, keeps):
        z = np.load(out_dir / (tag + ".npz"))
        res.append((case, fmt, keep, w, z["ids"], z["dists"], timing[tag]))
    return res


def _check_answers(case, fmt, keep, ids, dists, t):
    """The requested engine, the rotation flag, and answers bit-equal to the oracle's."""
    nodes, queries = SM.case_data(case)
    ref_ids, ref_d = _reference(case)
    engine, rot = ENGINE[fmt]
    assert t["engine"] == engine, (case.name, fmt, t)
    if rot is not None:
        assert bool(t["flags"] & HVS_TIMING_I8_ROTATED) == (rot == "1"), (case.name, fmt, t)
    assert np.array_equal(np.sort(dists, axis=1).view(np.uint32), ref_d[keep].view(np.uint32)), (case.name, fmt)
    with T.oracle_k(case.k):
        T.check_parity(nodes, queries[keep], ids, ref_ids[keep], case.sp, got_dists=dists)


def _check_reruns(case, fmt, regime, keep, w, t):
    """retry_queries / fallback_queries and the two re-run lists against the model's sets (indices of the call sent)."""
    want_retry = np.nonzero(w["retry"][keep])[0].tolist()
    want_exact = np.nonzero(w["exact"][keep])[0].tolist()
    if regime == "proven":
        assert t["retry"] == 0 and not want_retry, (case.name, fmt, t["retry"], want_retry)
    assert sorted(t["retry_list"]) == want_retry and t["retry"] == len(want_retry), (case.name, fmt, regime, sorted(t["retry_list"]), want_retry)
    assert sorted(t["exact_list"]) == want_exact and t["fallback"] == len(want_exact), (case.name, fmt, regime, sorted(t["exact_list"]), want_exact)


@pytest.mark.parametrize("shape", ["16", "32"])
@pytest.mark.parametrize("regime", ["proven", "default", "reckless"])
def test_production_counts_lie_in_the_model_bracket(work_dir, regime, shape):
    results = _run(work_dir, regime, shape)
    bad = []
    for case, fmt, keep, w, ids, dists, t in results:
        _check_answers(case, fmt, keep, ids, dists, t)
    for case, fmt, keep, w, ids, dists, t in results:
        lo, hi = SM.totals(w)
        inside = lo <= t["rescored"] <= hi
        print("%-8s I8_SHAPE=%s %-7s %-6s rescored %7d  model [%7d, %7d]  retried %2d (model %2d)  exact %d (model %d)  sent %d%s"
              % (regime, shape, case.name, fmt, t["rescored"], lo, hi, t["retry"], int(w["retry"][keep].sum()), t["fallback"],
                 int(w["exact"][keep].sum()), keep.size, "" if inside else "   <-- OUTSIDE"))
        _check_reruns(case, fmt, regime, keep, w, t)
        if not inside:
            bad.append((case.name, fmt, t["rescored"], lo, hi))
    assert not bad, bad


# --------------------------------------------------------------------------- caps, cursors and a row mask

_CHILD_ATTACHED = r"""
import importlib, json, os, sys, numpy as np
sys.path.insert(0, '.')
PKG = importlib.import_module('project---hybrid-vector-search-queries_amd')
spec = json.loads(sys.argv[1])
out = {}
for data, engine, rot, k, sp, cells in spec['engines']:
    z = np.load(os.path.join(spec['dir'], data + '.npz'))
    if rot is None:
        os.environ.pop('HVS_I8_ROTATE', None)
    else:
        os.environ['HVS_I8_ROTATE'] = rot
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(k)
        e.load_data(z['nodes'])
        e.reserve(spec['reserve'])
        masked = False
        if os.path.exists(os.path.join(spec['dir'], data + '.sets.npy')):      # the case's row sets, all of them, once per engine
            e.set_row_sets(np.load(os.path.join(spec['dir'], data + '.sets.npy')))
        for tag in cells:      # (the cells with a mask come last: the mask is set once and stays)
            get = lambda part: np.load(os.path.join(spec['dir'], tag + '.' + part + '.npy')) if os.path.exists(os.path.join(spec['dir'], tag + '.' + part + '.npy')) else None
            keep, caps, after_d, after_i, live = get('keep'), get('caps'), get('after_d'), get('after_i'), get('live')
            ex_off, ex_ids, set_idx = get('ex_off'), get('ex_ids'), get('set_idx')
            lists = None if ex_off is None else [ex_ids[ex_off[q]:ex_off[q + 1]] for q in keep]      # the CSR cut to `keep`
            assert not (masked and live is None)
            if live is not None and not masked:
                e.set_row_mask(live)
                masked = True
            if set_idx is None:
                ids, d = e.query(z['queries'][keep], sp, max_dist2=None if caps is None else caps[keep],
                                 after=None if after_d is None else (after_d[keep], after_i[keep]), exclude=lists)
            elif caps is None and after_d is None and lists is None:
                ids, d = e.query(z['queries'][keep], sp, row_set=set_idx[keep])
            else:                  # (row_set= stands alone in one call: the others are attached to the resident queries)
                e.upload_queries(z['queries'][keep])
                if caps is not None:
                    e.set_max_dist2(caps[keep])
                if after_d is not None:
                    e.set_after(after_d[keep], after_i[keep])
                if lists is not None:
                    e.set_exclude_ids(lists)
                e.set_query_row_sets(set_idx[keep])
                e.query_resident(0, keep.size, sp)
                e.sync()
                ids, d = e.download_results(0, keep.size)
            t = e.last_timing()
            reruns = [e.last_reruns(0).tolist(), e.last_reruns(1).tolist()]
            m, w, a, x, r = e.mask_stats(), e.within_stats(), e.after_stats(), e.exclude_stats(), e.row_sets_stats()
            np.savez(os.path.join(spec['out'], tag + '.npz'), ids=ids, dists=d)
            out[tag] = dict(engine=int(t.engine), fallback=int(t.fallback_queries), retry=int(t.retry_queries), flags=int(t.flags),
                            rescored=int(t.rescored_pairs), exact_list=reruns[0], retry_list=reruns[1], dead_survivors=int(m.dead_survivors),
                            n_dead=int(m.n_dead), within=w.as_dict(), after=a.as_dict(), exclude=x.as_dict(), row_sets=r.as_dict())
print('RESULT ' + json.dumps(out))
"""
_MASK_LAST = {name: (name in ("mask", "all", "ex_all", "rs_all"), i) for i, name in enumerate(SM.ATTACH)}


def _run_attached(work_dir, regime, shape, lib=None):
    """One child: every attached cell of (regime, HVS_I8_SHAPE, library), one engine per (case, format), its cells one call each.
    Returns [(case, fmt, name, attachment, keep, production walk, ids, dists, counts)]."""
    cells = SM.attach_cells(regime, shape, lib is not None)
    label = "%s-attached-%s-%s" % ("wide" if lib else "production", regime, shape)
    out_dir = work_dir / label
    out_dir.mkdir(exist_ok=True)
    engines, runs = {}, []
    for case, fmt, _, name in sorted(cells, key=lambda c: (c[0].name, c[1], _MASK_LAST[c[3]])):
        att = SM.attachment(case, name)
        w = SM.case_walk(case, fmt, regime, attach=name)         # the production model decides what is sent, for either library
        keep = np.nonzero(~w["excluded"])[0]
        tag = "%s-%s-%s-%s" % (label, case.name, fmt, name)
        np.save(work_dir / (tag + ".keep.npy"), keep)
        if "caps" in att:
            np.save(work_dir / (tag + ".caps.npy"), att["caps"])
        if "after" in att:
            np.save(work_dir / (tag + ".after_d.npy"), att["after"][0])
            np.save(work_dir / (tag + ".after_i.npy"), att["after"][1])
        if "live" in att:
            np.save(work_dir / (tag + ".live.npy"), att["live"])
        if "excl" in att:
            import exclude_model as XM
            off, ex_ids = XM.csr(att["excl"])
            np.save(work_dir / (tag + ".ex_off.npy"), off)
            np.save(work_dir / (tag + ".ex_ids.npy"), ex_ids)
        if "sets" in att:
            if not (work_dir / (case.name + ".sets.npy")).exists():
                np.save(work_dir / (case.name + ".sets.npy"), SM.case_set_table(case)[0])
            np.save(work_dir / (tag + ".set_idx.npy"), SM.table_indices(case, name))
        engine, rot = ENGINE[fmt]
        engines.setdefault((case.name, engine, rot, case.k, case.sp), []).append(tag)
        runs.append((case, fmt, name, att, keep, w, tag))
    env = dict(os.environ, HVS_I8_SHAPE=shape)
    for var in ("HVS_I8_ROTATE", "HVS_LIB", "HVS_GUESS_MID", "HVS_GUESS_PFAIL", "HVS_RADICES"):
        env.pop(var, None)
    env.update(SM.REGIMES[regime]["env"])
    if lib:
        env["HVS_LIB"] = lib
    spec = dict(dir=str(work_dir), out=str(out_dir), engines=[list(key) + [tags] for key, tags in engines.items()], reserve=SM.RESERVE_NQ)
    counts = T.run_child(_CHILD_ATTACHED, spec, env, label, CHILD_TIMEOUT)
    res = []
    for case, fmt, name, att, keep, w, tag in runs:
        z = np.load(out_dir / (tag + ".npz"))
        res.append((case, fmt, name, att, keep, w, z["ids"], z["dists"], counts[tag]))
    return res


_expected = {}


def _check_attached_answers(case, fmt, name, att, keep, ids, dists, t):
    """The requested engine, the rotation flag, answers equal to the attachment's expected ones in ids and distance bits (the key
    order is total: nothing is loosened for ties, as in tests/test_after.py), and the features' own counts of those answers."""
    if (case.name, name) not in _expected:
        _expected[(case.name, name)] = SM.expected_answers(case, att)
    ref_ids, ref_d, matched = _expected[(case.name, name)]
    engine, rot = ENGINE[fmt]
    where = (case.name, fmt, name)
    assert t["engine"] == engine, (where, t)
    if rot is not None:
        assert bool(t["flags"] & HVS_TIMING_I8_ROTATED) == (rot == "1"), (where, t)
    bad = np.nonzero((dists.view(np.uint32) != ref_d[keep].view(np.uint32)).any(1) | (ids != ref_ids[keep]).any(1))[0]
    assert bad.size == 0, (where, "queries (of those sent) with another answer:", bad[:10].tolist())
    slots, underfull = int(matched[keep].sum()), int((matched[keep] < case.k).sum())
    if "caps" in att:
        assert (t["within"]["within_slots"], t["within"]["underfull_queries"]) == (slots, underfull), (where, t["within"], slots, underfull)
    if "after" in att:
        exhausted = int((att["after"][1][keep] == 0xFFFFFFFF).sum())
        assert (t["after"]["after_slots"], t["after"]["underfull_queries"], t["after"]["exhausted_queries"]) == (slots, underfull, exhausted), \
            (where, t["after"], slots, underfull, exhausted)
    assert t["n_dead"] == (int((~att["live"]).sum()) if "live" in att else 0), (where, t["n_dead"])
    r = t["row_sets"]
    if "sets" in att:
        restricted = int((att["sets"][1][keep] != SM.SET_NONE).sum())
        assert (r["restricted_queries"], r["kept_slots"], r["underfull_queries"]) == (restricted, slots, underfull), (where, r, restricted, slots, underfull)
    else:
        assert (r["restricted_queries"], r["kept_slots"], r["underfull_queries"], r["refused_keys"]) == (0, 0, 0, 0), (where, r)
    x = t["exclude"]
    if "excl" in att:
        assert (x["excluding_queries"], x["kept_slots"], x["underfull_queries"]) == (keep.size, slots, underfull), (where, x, keep.size, slots, underfull)
    else:
        assert x == dict(excluding_queries=0, underfull_queries=0, kept_slots=0, refused_keys=0), (where, x)


def _check_refused(case, fmt, name, att, keep, w, t, bad):
    """hvs_exclude_info.refused_keys against the model's `refused`: equal where the filter answers every query; with an exact
    fallback (the `out` cells) at least the filter-answered queries' sum and strictly above it -- the fallback queries list
    matched rows, which only the re-run sink (counter slot 26) can have refused.
    Under row sets hvs_row_sets_info.refused_keys against the model's `set_refused` by the same rule (the sink's slot 36)."""
    sink = bool(w["exact"][keep].any())
    line = ""
    for part, stats, model in (("excl", "exclude", "refused"), ("sets", "row_sets", "set_refused")):
        if part not in att:
            continue
        got, want = t[stats]["refused_keys"], int(w[model][keep].sum())
        if (got <= want) if sink else (got != want):
            bad.append((case.name, fmt, name, stats + " refused_keys", got, "above" if sink else "equal to", want))
        line += "  %s %6d (model %s%d)" % (model, got, "> " if sink else "", want)
    return line


def _check_page2_twin(results, bad):
    """DESIGN 3.14's "the same re-scored pairs": in one child, on one engine, the ex_p1 cell re-scores exactly the pairs the
    after_p2 cell does and retries the same queries -- measured against measured.  The rs_page1 cell, whose sets are the complements
    of ex_p1's lists, against the ex_p1 cell likewise, and its refused keys (the set's counter) equal to ex_p1's (the list's).
    Returns the number of (ex_p1, after_p2) pairs; every rs_page1 cell must have found its ex_p1."""
    cells = {(case.name, fmt, name): (keep, t) for case, fmt, name, att, keep, w, ids, dists, t in results}
    twins = 0
    for (cname, fmt, name), (keep, t) in cells.items():
        other = {"ex_p1": "after_p2", "rs_page1": "ex_p1"}.get(name)
        if other is None:
            continue
        if (cname, fmt, other) not in cells:
            assert name != "rs_page1", (cname, fmt, "an rs_page1 cell without its ex_p1 cell in the child")
            continue
        keep2, t2 = cells[(cname, fmt, other)]
        twins += name == "ex_p1"
        same_sent = np.array_equal(keep, keep2)
        print("%-7s %-6s %s rescored %7d retried %s  %s rescored %7d retried %s" % (
            cname, fmt, name, t["rescored"], sorted(t["retry_list"]), other, t2["rescored"], sorted(t2["retry_list"])))
        if not (same_sent and t["rescored"] == t2["rescored"] and sorted(t["retry_list"]) == sorted(t2["retry_list"])):
            bad.append((cname, fmt, name + " against " + other, t["rescored"], t2["rescored"], sorted(t["retry_list"]), sorted(t2["retry_list"])))
        if name == "rs_page1" and t["row_sets"]["refused_keys"] != t2["exclude"]["refused_keys"]:
            bad.append((cname, fmt, "rs_page1's set refusals against ex_p1's list refusals", t["row_sets"]["refused_keys"], t2["exclude"]["refused_keys"]))
    return twins


def _attached_line(label, case, fmt, name, t, lo, hi, dlo, dhi, keep, w, ok):
    return "%-18s %-7s %-6s %-10s rescored %7d  model [%7d, %7d]  dead %5d [%5d, %5d]  retried %2d (model %2d)  exact %d  sent %d%s" % (
        label, case.name, fmt, name, t["rescored"], lo, hi, t["dead_survivors"], dlo, dhi, t["retry"], int(w["retry"][keep].sum()),
        t["fallback"], keep.size, "" if ok else "   <-- OUTSIDE")


@pytest.mark.parametrize("regime,shape", [("proven", "16"), ("default", "16"), ("reckless", "16"), ("default", "32")])
def test_attached_counts_lie_in_the_model_bracket(work_dir, regime, shape):
    """Caps, cursors, a row mask, exclusion lists and shared row sets (selectivity_model.ATTACH over ATTACH_MATRIX): answers and the
    features' own counts first, then retry and exact lists exactly, rescored_pairs and dead_survivors inside the model's brackets,
    both refused_keys equal to the model's, and the ex_p1 cells against the after_p2 cells, the rs_page1 cells against the ex_p1
    cells, measured in the same child."""
    results = _run_attached(work_dir, regime, shape)
    for case, fmt, name, att, keep, w, ids, dists, t in results:
        _check_attached_answers(case, fmt, name, att, keep, ids, dists, t)
    bad = []
    for case, fmt, name, att, keep, w, ids, dists, t in results:
        (lo, hi), (dlo, dhi) = SM.totals(w), SM.totals(w, what="dead_")
        inside = lo <= t["rescored"] <= hi and dlo <= t["dead_survivors"] <= dhi
        print(_attached_line("%s I8_SHAPE=%s" % (regime, shape), case, fmt, name, t, lo, hi, dlo, dhi, keep, w, inside)
              + _check_refused(case, fmt, name, att, keep, w, t, bad))
        _check_reruns(case, fmt + "/" + name, regime, keep, w, t)
        if not inside:
            bad.append((case.name, fmt, name, t["rescored"], lo, hi, t["dead_survivors"], dlo, dhi))
    twins = _check_page2_twin(results, bad)
    assert twins >= 1, "no (ex_p1, after_p2) pair in this child"
    assert not bad, bad


def test_a_band_too_wide_is_seen_under_attachments(work_dir, wide_band_lib):
    """The band x 1.25 build under cap_kth, after_p2, mask, ex_p1 and rs_half: right answers, above the production bracket, inside the model's
    bracket for that band."""
    results = _run_attached(work_dir, "default", "16", lib=wide_band_lib)
    for case, fmt, name, att, keep, w, ids, dists, t in results:
        _check_attached_answers(case, fmt, name, att, keep, ids, dists, t)
    bad = []
    for case, fmt, name, att, keep, w, ids, dists, t in results:
        m = SM.case_walk(case, fmt, "default", SM.MUTANT_SCALE, attach=name)
        lo, hi = SM.totals(w)
        (mlo, mhi), (dlo, dhi) = SM.totals(m, ~w["excluded"]), SM.totals(m, ~w["excluded"], what="dead_")
        ok = hi < t["rescored"] and mlo <= t["rescored"] <= mhi and dlo <= t["dead_survivors"] <= dhi
        print(_attached_line("band x %.2f" % SM.MUTANT_SCALE, case, fmt, name, t, mlo, mhi, dlo, dhi, keep, m, ok) + "  production model [%d, %d]" % (lo, hi)
              + _check_refused(case, fmt, name, att, keep, m, t, bad))
        _check_reruns(case, fmt + "/" + name, "default", keep, m, t)
        if not ok:
            bad.append((case.name, fmt, name, t["rescored"], (lo, hi), (mlo, mhi)))
    assert _check_page2_twin(results, bad) == 2
    assert not bad, bad


@pytest.mark.parametrize("regime", ["proven", "default"])
def test_a_band_too_wide_is_seen(work_dir, wide_band_lib, regime):
    """-DHVS_MUTANT_BAND_SCALE=1.25 answers correctly and re-scores more than the production bracket allows."""
    results = _run(work_dir, regime, "16", lib=wide_band_lib)
    for case, fmt, keep, w, ids, dists, t in results:
        _check_answers(case, fmt, keep, ids, dists, t)
    bad = []
    for case, fmt, keep, w, ids, dists, t in results:
        m = SM.case_walk(case, fmt, regime, SM.MUTANT_SCALE)
        lo, hi = SM.totals(w)
        mlo, mhi = SM.totals(m, ~w["excluded"])
        ok = hi < t["rescored"] and mlo <= t["rescored"] <= mhi
        print("band x %.2f %-8s %-7s %-6s rescored %7d  production model [%7d, %7d]  model of the wide band [%7d, %7d]%s"
              % (SM.MUTANT_SCALE, regime, case.name, fmt, t["rescored"], lo, hi, mlo, mhi, "" if ok else "   <-- NOT AS MODELLED"))
        _check_reruns(case, fmt, regime, keep, m, t)
        if not ok:
            bad.append((case.name, fmt, t["rescored"], (lo, hi), (mlo, mhi)))
    assert not bad, bad
