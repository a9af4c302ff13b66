"""What a call leaves behind on one GPU, as a pure function (DESIGN 3.5a "What a call leaves behind"): the states of the host's
HvsCallState restated over four facts -- whether there is a last call to report, whether its re-runs may still be pending,
which queries hvs_last_reruns names, and whether the call ran under a live-row mask.  tests/test_callstate_walk.py walks one
context through the calls below and compares what the library reports after each with `report`.

A call is a tuple:
    ("run", q0, nq)        hvs_query_resident of resident queries [q0, q0 + nq)
    ("query",)             hvs_query of all queries: enqueued, resolved and fetched in one call
    ("read",)              anything through which results or figures leave (hvs_download_results, hvs_sync, hvs_last_timing,
                           hvs_last_reruns, the *_stats calls): pending re-runs are resolved first
    ("set_k", k)           hvs_set_k
    ("set_engine", e)      hvs_set_engine on a context whose orderings exist: FILTER or EXACT (below)
    ("delete", count)      hvs_delete_rows of `count` live rows
    ("compact",)           hvs_compact

`retry` and `exact` of `initial` are the sets of tests/selectivity_model.py for the queries sent: the queries whose guessed
threshold fails its check, and those without a usable INT8 bound.  A call names the members inside its own range, by their
resident index.

Cells that are easy to get wrong, each read from the code and seen on the GPU before HvsCallState existed:
  - hvs_last_reruns does not ask whether there is a last call to report: after hvs_set_k and after hvs_compact it still returns
    the LENGTHS of the forgotten call's lists while hvs_last_timing returns HVS_ESTATE.  After hvs_set_k the indices themselves
    are gone (the lists are re-allocated with the result rows); `lists_kept` says whether they can be compared.
  - a call begins by resolving the call before it: two hvs_query_resident calls in a row lose nothing of the first, and the
    lists reported afterwards are the second call's alone.
  - hvs_set_engine on a context that has orderings builds nothing and runs no planner probe (the probe belongs to an index
    build under HVS_ENGINE_AUTO): the last call's report, its lists and its pending re-runs all survive AUTO and back.
  - deleting rows forgets nothing: the last call can still be asked for, and its dead_survivors stay zero.
  - hvs_mask_info.dead_survivors is zero after a masked call too: the tiles carry tombstones for the dead rows, so no dead row
    survives a filter (tests/test_row_mask.py pins that); what tells a masked call here is hvs_mask_info.n_dead.
  - under a mask the model's sets no longer apply (distances to dead rows left the thresholds): `lists_known` is false.
  - an exact-engine call has no lists; the filter call's are not reported after it."""
from collections import namedtuple

OK, ESTATE = 0, -4
FILTER, EXACT = "filter", "exact"

# valid: there is a last call to report;  pending: its re-runs may not have run yet
# exact / retry: what hvs_last_reruns(0 | 1) names (sorted resident indices);  lists_kept: the indices are still on the device
# lists_known: the model can say which they are;  engine: what the next call runs on;  dead: rows deleted and not compacted away
# call_engine: what the last call ran on (None: none to report)
State = namedtuple("State", "retry_all exact_all valid pending exact retry lists_kept lists_known engine dead call_engine k")


def initial(retry, exact, k, engine=FILTER):
    return State(tuple(sorted(retry)), tuple(sorted(exact)), False, False, (), (), True, True, engine, 0, None, k)


def _called(s, q0, nq, pending):
    if s.engine == EXACT:
        return s._replace(valid=True, pending=False, exact=(), retry=(), lists_kept=True, lists_known=True, call_engine=EXACT)
    inside = lambda idx: tuple(i for i in idx if q0 <= i < q0 + nq)
    return s._replace(valid=True, pending=pending, exact=inside(s.exact_all), retry=inside(s.retry_all), lists_kept=True,
                      lists_known=s.dead == 0, call_engine=FILTER)


def step(s, call):
    op = call[0]
    if op == "run":
        return _called(s, call[1], call[2], True)
    if op == "query":
        return _called(s, 0, 1 << 32, False)
    if op == "read":
        return s._replace(pending=False)
    if op == "set_k":
        if call[1] == s.k:
            return s
        return s._replace(k=call[1], valid=False, pending=False, lists_kept=False, call_engine=None)
    if op == "set_engine":
        return s._replace(engine=call[1])
    if op == "delete":
        return s._replace(pending=False, dead=s.dead + call[1])
    if op == "compact":
        return s._replace(valid=False, pending=False, dead=0, call_engine=None)
    raise ValueError(f"unknown call {call!r}")


def report(s):
    """What the library says once the pending re-runs have run: the status of hvs_last_timing, the lengths of the two lists,
    the lists themselves (None: not comparable) and retry_queries / fallback_queries of hvs_last_timing (None with ESTATE)."""
    lists = (s.exact, s.retry) if s.lists_kept and s.lists_known else None
    lengths = (len(s.exact), len(s.retry)) if s.lists_known else None
    return dict(timing=OK if s.valid else ESTATE, lengths=lengths, lists=lists,
                counts=(lengths if s.valid else None), engine=s.call_engine)
