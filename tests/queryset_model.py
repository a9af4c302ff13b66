"""What is attached to the resident queries, as a pure function (DESIGN 3.13a "Resident-query state"): the transition table
of the host's HvsQuerySet restated over four facts -- category sets, distance caps, result cursors, and whether every resident
query has a result row at the current k -- and a fifth beside them: whether the last call's figures can still be asked for.
Three more facts take the staged attach (exclusion lists, candidate lists, per-query indices of the shared row sets), and the
shared row sets themselves stand beside them: they are the data set's, not the queries'.
The expanded resident set has three clients -- category sets, extra query vectors, extra clauses -- and one at a time: the fact
is the pair (kind, tag), kept as the fields `kind` and `sets` (`expanded` returns the pair), so that "sets" stays the tag it was.
tests/test_queryset_model_cpu.py pins the table row by row; tests/test_queryset_walk.py walks one GPU context through it and
compares every answer with a fresh context given only what the model says is attached.

A call is a tuple:
    ("upload", tag)            hvs_upload_queries of the query rows named `tag`
    ("query", tag)             hvs_query: the same, and all of them answered
    ("sets", tag | None)       hvs_set_category_sets (None: detach)
    ("bad_sets",)              ... with sets the library refuses (HVS_EINVAL)
    ("vectors", tag | None)    hvs_set_query_vectors (None: detach)
    ("clauses", tag | None)    hvs_set_query_clauses; tag = (name, whether the clauses bring vectors of their own)
    ("bad_vectors", ...)       ... with offsets the library refuses (HVS_EINVAL); what follows the name says which, for the walk
    ("bad_clauses", ...)
    ("caps", tag | None)       hvs_set_max_dist2
    ("after", tag | None)      hvs_set_after
    ("after_from_results",)    hvs_set_after_from_results (padding off)
    ("set_k", k)               hvs_set_k
    ("run", q0, nq)            hvs_query_resident
    ("exclude", tag | None)    hvs_set_exclude_ids (None: remove)
    ("bad_exclude",)           ... with offsets the library refuses (HVS_EINVAL)
    ("candidates", tag | None) hvs_set_candidate_ids; HVS_ESTATE while a client of the expanded set is attached
    ("bad_candidates",)        ... with offsets the library refuses
    ("row_sets", tag | None)   hvs_set_row_sets: the shared sets loaded, replaced or (None) removed
    ("query_sets", tag | None) hvs_set_query_row_sets; HVS_ESTATE while no shared sets are loaded
    ("bad_query_sets",)        ... with an index that names no set

`step` returns the next state and the call's status: OK, EINVAL or ESTATE.  A refused call leaves the state as it was.

Three cells of the table that are easy to get wrong, read from the code:
  - detaching sets from a context that has none is a no-op: caps, cursors and results stay;
  - caps and cursors survive hvs_set_k, the results do not;
  - attaching or removing caps or cursors leaves the result range alone (the rows are still those of the earlier call), so
    hvs_set_after_from_results may follow them.
The clients' rows: an attach of any client replaces whichever is attached and drops caps, cursors, lists, set indices, results and
the last call's figures; X(None) detaches X and drops the same, and is a no-op -- nothing dropped, the results stay -- while another
client is attached or none is; a refused attach changes nothing.  While a row can come back under several keys -- extra vectors,
or clauses that bring vectors -- cursors are refused (HVS_ESTATE, asked before the values and before the results) and may still
be removed; category sets and predicate-only clauses allow them.
The lists' rows: a replaced resident set and category sets attached or detached drop all three kinds; replacing the shared sets
drops the indices (they named the old sets) and the results, and nothing else; lists and indices leave the result range alone, as
caps do; removing cursors under lists or indices leaves them in force; the state is checked before the values are, so a call
that is both out of place and malformed is HVS_ESTATE.
The result range is one interval: a call's range joins it when the two touch and replaces it otherwise.  (A multi-GPU context
keeps one interval per GPU, in that GPU's own query numbers: the walks stay clear of sequences where that shows.  The library
tells a k that changed by comparing the range's k with the current one, so k -> k' -> k without a call in between would find
the old range again; the model calls the results gone, and no walk goes there.)"""
from collections import namedtuple

OK, EINVAL, ESTATE = 0, -1, -4
FROM_RESULTS = "from results"   # cursors: the last slot of each query's current result row

# queries: tag of the resident rows; nq: their number; sets / caps / cursors: tag of what is attached (None: nothing);
# k: slots per result row; res: the answered interval (lo, hi) at this k, or None
# timed: the last call's figures (hvs_last_timing, hvs_within_stats, ...) can be asked for
# excl / cand / qsets: tag of the exclusion lists, candidate lists, set indices attached; rsets: tag of the shared row sets loaded
# kind: the client that `sets` is the tag of -- one of CLIENTS; "sets" while none is attached
State = namedtuple("State", "queries nq sets caps cursors k res timed excl cand qsets rsets kind",
                   defaults=[True, None, None, None, None, "sets"])
CLIENTS = ("sets", "vectors", "clauses")


def initial(k=100):
    return State(None, 0, None, None, None, k, None, False)


def full(s):
    """every resident query has a result row at the current k (what hvs_set_after_from_results needs); at least one query"""
    return s.res is not None and s.res[0] == 0 and s.res[1] >= s.nq


def expanded(s):
    """the expanded set's client: (kind, tag), or None"""
    return None if s.sets is None else (s.kind, s.sets)


def many_keys(s):
    """a row can come back under several keys: cursors are refused"""
    return s.sets is not None and (s.kind == "vectors" or (s.kind == "clauses" and bool(s.sets[1])))


def _answered(s, q0, nq):
    lo, hi = q0, q0 + nq
    if s.res is not None and s.res[0] < s.res[1] and not (lo > s.res[1] or hi < s.res[0]):
        lo, hi = min(lo, s.res[0]), max(hi, s.res[1])
    return s._replace(res=(lo, hi), timed=True)


def step(s, call, nq_of=None):
    """(state, call) -> (state, status).  `nq_of`: tag -> number of query rows (for "upload" / "query")."""
    op = call[0]
    if op in ("upload", "query"):
        n = nq_of[call[1]] if nq_of else s.nq
        s = s._replace(queries=call[1], nq=n, sets=None, kind="sets", caps=None, cursors=None, res=None, excl=None, cand=None, qsets=None)
        return (_answered(s, 0, n) if op == "query" else s), OK
    if op in CLIENTS:
        if call[1] is None and (s.sets is None or s.kind != op):
            return s, OK
        return s._replace(sets=call[1], kind="sets" if call[1] is None else op, caps=None, cursors=None, res=None, timed=False, excl=None,
                          cand=None, qsets=None), OK
    if op.startswith("bad_") and op[4:] in CLIENTS:
        return s, EINVAL
    if op == "caps":
        return s._replace(caps=call[1]), OK
    if op == "after":
        return (s, ESTATE) if call[1] is not None and many_keys(s) else (s._replace(cursors=call[1]), OK)
    if op == "after_from_results":
        return (s._replace(cursors=FROM_RESULTS), OK) if full(s) and not many_keys(s) else (s, ESTATE)
    if op == "set_k":
        return (s, OK) if call[1] == s.k else (s._replace(k=call[1], res=None, timed=False), OK)
    if op == "run":
        if call[1] + call[2] > s.nq:
            return s, EINVAL
        return _answered(s, call[1], call[2]), OK
    if op == "exclude":
        return s._replace(excl=call[1]), OK
    if op == "bad_exclude":
        return s, EINVAL
    if op in ("candidates", "bad_candidates"):
        if op == "candidates" and call[1] is None:
            return s._replace(cand=None), OK
        if s.sets is not None:
            return s, ESTATE
        return (s._replace(cand=call[1]), OK) if op == "candidates" else (s, EINVAL)
    if op == "row_sets":
        return s._replace(rsets=call[1], qsets=None, res=None), OK
    if op in ("query_sets", "bad_query_sets"):
        if op == "query_sets" and call[1] is None:
            return s._replace(qsets=None), OK
        if s.rsets is None:
            return s, ESTATE
        return (s._replace(qsets=call[1]), OK) if op == "query_sets" else (s, EINVAL)
    raise ValueError(f"unknown call {call!r}")
