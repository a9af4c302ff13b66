"""The transition table of the resident-query state, pinned row by row on tests/queryset_model.py."""
import pytest

import queryset_model as M

NQ = {"Q": 80, "Q2": 80, "short": 30}
EVERYTHING = M.State("Q", 80, "S", "C", "A", 8, (0, 80))       # sets, caps, cursors, full results
PLAIN_FULL = M.State("Q", 80, None, None, None, 8, (0, 80))


def go(s, *calls):
    for call in calls:
        s, rc = M.step(s, call, NQ)
        assert rc == M.OK, call
    return s


def attached(s):
    return (s.sets, s.caps, s.cursors, M.full(s))


def test_the_start():
    s = M.initial()
    assert attached(s) == (None, None, None, False) and s.k == 100 and not s.timed


@pytest.mark.parametrize("call", [("upload", "Q2"), ("upload", "short")])
def test_row_resident_set_replaced(call):
    s = go(EVERYTHING, call)
    assert attached(s) == (None, None, None, False)
    assert (s.queries, s.nq, s.k) == (call[1], NQ[call[1]], 8)
    assert s.timed                                               # (the last call's figures outlive its queries)


def test_row_hvs_query_replaces_the_set_and_answers_it():
    s = go(EVERYTHING, ("query", "short"))
    assert attached(s) == (None, None, None, True) and s.nq == 30


def test_row_sets_attached():
    s = go(EVERYTHING, ("sets", "S2"))
    assert attached(s) == ("S2", None, None, False) and not s.timed
    s = go(M.State("Q", 80, None, "C", "A", 8, (0, 80)), ("sets", "S"))
    assert attached(s) == ("S", None, None, False)


def test_row_sets_detached():
    s = go(EVERYTHING, ("sets", None))
    assert attached(s) == (None, None, None, False) and not s.timed


def test_row_detach_without_sets_is_a_no_op():
    s = M.State("Q", 80, None, "C", "A", 8, (0, 80))
    assert go(s, ("sets", None)) == s


def test_row_refused_sets_change_nothing():
    for s in (EVERYTHING, PLAIN_FULL, M.initial()):
        assert M.step(s, ("bad_sets",), NQ) == (s, M.EINVAL)


def test_rows_caps_and_cursors_touch_only_themselves():
    s = go(EVERYTHING, ("caps", "C2"))
    assert s == EVERYTHING._replace(caps="C2")
    s = go(EVERYTHING, ("caps", None))
    assert s == EVERYTHING._replace(caps=None)
    s = go(EVERYTHING, ("after", "A2"))
    assert s == EVERYTHING._replace(cursors="A2")
    s = go(EVERYTHING, ("after", None))
    assert s == EVERYTHING._replace(cursors=None)


def test_row_k_changed():
    s = go(EVERYTHING, ("set_k", 100))
    assert attached(s) == ("S", "C", "A", False) and s.k == 100 and not s.timed
    assert go(s, ("run", 0, 80)).timed
    assert go(EVERYTHING, ("set_k", 8)) == EVERYTHING            # (the same k: nothing happens)


def test_row_call_answered_joins_or_replaces():
    s = go(PLAIN_FULL, ("upload", "Q"))
    s = go(s, ("run", 20, 30))
    assert s.res == (20, 50) and not M.full(s)
    assert go(s, ("run", 50, 30)).res == (20, 80)                # touches at the end: joined
    assert go(s, ("run", 0, 20)).res == (0, 50)                  # touches at the start: joined
    assert go(s, ("run", 30, 40)).res == (20, 70)                # overlaps: joined
    assert go(s, ("run", 60, 20)).res == (60, 80)                # apart: replaced
    assert go(s, ("run", 0, 10)).res == (0, 10)
    t = go(s, ("run", 50, 30), ("run", 0, 20))
    assert t.res == (0, 80) and M.full(t)
    assert attached(go(EVERYTHING, ("run", 10, 5))) == ("S", "C", "A", True)   # a call keeps what is attached, and the rows it had
    assert M.step(PLAIN_FULL, ("run", 70, 11), NQ) == (PLAIN_FULL, M.EINVAL)


def test_row_cursors_from_results():
    s, rc = M.step(EVERYTHING, ("after_from_results",), NQ)
    assert rc == M.OK and s == EVERYTHING._replace(cursors=M.FROM_RESULTS)
    for t in (go(EVERYTHING, ("set_k", 100)), go(EVERYTHING, ("sets", None)), go(EVERYTHING, ("upload", "Q")),
              go(PLAIN_FULL, ("upload", "Q"), ("run", 20, 30)), M.initial()._replace(queries="Q", nq=80)):
        assert M.step(t, ("after_from_results",), NQ) == (t, M.ESTATE)
    # caps and cursors do not take the results away
    assert M.step(go(PLAIN_FULL, ("caps", "C"), ("after", "A")), ("after_from_results",), NQ)[1] == M.OK


LISTED = EVERYTHING._replace(excl="E", qsets="I", rsets="R")        # what composes with category sets
AMONG = PLAIN_FULL._replace(caps="C", cursors="A", excl="E", cand="K", qsets="I", rsets="R")


def lists(s):
    return (s.excl, s.cand, s.qsets, s.rsets)


@pytest.mark.parametrize("call", [("upload", "Q2"), ("query", "short")])
def test_row_resident_set_replaced_drops_the_lists(call):
    assert lists(go(AMONG, call)) == (None, None, None, "R")    # (the shared sets are the data set's: they stay)
    assert lists(go(LISTED, call)) == (None, None, None, "R")


def test_row_sets_changed_drops_the_lists():
    for call in (("sets", "S2"), ("sets", None)):
        assert lists(go(LISTED, call)) == (None, None, None, "R")
    assert lists(go(AMONG, ("sets", "S"))) == (None, None, None, "R")
    assert go(AMONG, ("sets", None)) == AMONG                    # (detaching nothing: a no-op for the lists too)


@pytest.mark.parametrize("fact, call", [("excl", "exclude"), ("cand", "candidates"), ("qsets", "query_sets")])
def test_rows_lists_touch_only_themselves(fact, call):
    assert go(AMONG, (call, "X")) == AMONG._replace(**{fact: "X"})
    assert go(AMONG, (call, None)) == AMONG._replace(**{fact: None})
    assert M.full(go(AMONG, (call, "X")))                        # the result range is left alone, as by caps


def test_row_candidates_do_not_compose_with_the_expanded_set():
    assert M.step(LISTED, ("candidates", "K"), NQ) == (LISTED, M.ESTATE)
    assert M.step(LISTED, ("bad_candidates",), NQ) == (LISTED, M.ESTATE)   # the state is asked before the offsets
    assert go(LISTED, ("candidates", None)) == LISTED            # removing is always allowed
    assert go(LISTED, ("exclude", "E2"), ("query_sets", "I2")) == LISTED._replace(excl="E2", qsets="I2")


def test_row_shared_sets_replaced():
    for call in (("row_sets", "R2"), ("row_sets", None)):
        s = go(AMONG, call)
        assert lists(s) == ("E", "K", None, call[1]) and s.res is None     # the indices named the old sets; the results go
        assert (s.sets, s.caps, s.cursors, s.timed) == (None, "C", "A", True)
    none = PLAIN_FULL
    assert M.step(none, ("query_sets", "I"), NQ) == (none, M.ESTATE)
    assert M.step(none, ("bad_query_sets",), NQ) == (none, M.ESTATE)
    assert go(none, ("query_sets", None)) == none


def test_row_removing_cursors_leaves_the_lists():
    assert go(AMONG, ("after", None)) == AMONG._replace(cursors=None)
    assert go(LISTED, ("after", None), ("caps", None)) == LISTED._replace(cursors=None, caps=None)


def test_row_refused_lists_change_nothing():
    for s in (AMONG, PLAIN_FULL._replace(rsets="R")):
        for call in (("bad_exclude",), ("bad_candidates",), ("bad_query_sets",)):
            assert M.step(s, call, NQ) == (s, M.EINVAL)
    assert M.step(LISTED, ("bad_exclude",), NQ) == (LISTED, M.EINVAL)


def test_row_k_changed_keeps_the_lists():
    s = go(AMONG, ("set_k", 100))
    assert lists(s) == lists(AMONG) and s.res is None


# ---- the expanded set's three clients: the fact is (kind, tag) ----
PREDICATES, WITH_VECTORS = ("P", False), ("W", True)                # clauses' tags say whether they bring vectors
CLIENT_TAGS = {"sets": "S2", "vectors": "X", "clauses": PREDICATES}
UNDER = {"sets": LISTED,                                            # everything that composes, under each client
         "vectors": LISTED._replace(sets="X", kind="vectors", cursors=None),
         "clauses": LISTED._replace(sets=PREDICATES, kind="clauses")}
DROPPED = dict(caps=None, cursors=None, res=None, timed=False, excl=None, cand=None, qsets=None)


def test_the_expanded_fact_is_kind_and_tag():
    assert M.expanded(PLAIN_FULL) is None and M.expanded(EVERYTHING) == ("sets", "S")
    assert M.expanded(UNDER["vectors"]) == ("vectors", "X") and M.expanded(UNDER["clauses"]) == ("clauses", PREDICATES)


@pytest.mark.parametrize("was", M.CLIENTS)
@pytest.mark.parametrize("client", M.CLIENTS)
def test_row_a_client_attached_replaces_whichever_is(client, was):
    tag = CLIENT_TAGS[client]
    for s in (UNDER[was], AMONG):
        assert go(s, (client, tag)) == s._replace(sets=tag, kind=client, **DROPPED)


@pytest.mark.parametrize("was", M.CLIENTS)
@pytest.mark.parametrize("client", M.CLIENTS)
def test_row_a_client_detached(client, was):
    s = UNDER[was]
    if client == was:
        assert go(s, (client, None)) == s._replace(sets=None, kind="sets", **DROPPED)
    else:
        assert go(s, (client, None)) == s                       # another client's detach: nothing dropped, the results stay
    assert go(AMONG, (client, None)) == AMONG                   # ... and so while none is attached


@pytest.mark.parametrize("client", M.CLIENTS)
def test_row_a_refused_client_changes_nothing(client):
    for s in (*UNDER.values(), AMONG, PLAIN_FULL, M.initial()):
        assert M.step(s, ("bad_" + client,), NQ) == (s, M.EINVAL)
        assert M.step(s, ("bad_" + client, "one list over the limit"), NQ) == (s, M.EINVAL)


def test_row_cursors_under_the_clients():
    several = (UNDER["vectors"], UNDER["vectors"]._replace(sets=WITH_VECTORS, kind="clauses"))
    for s in several:
        assert M.full(s)
        assert M.step(s, ("after", "A2"), NQ) == (s, M.ESTATE)
        assert M.step(s, ("after_from_results",), NQ) == (s, M.ESTATE)
        t = s._replace(res=None)                                 # the state is asked before the values
        assert M.step(t, ("after_from_results",), NQ) == (t, M.ESTATE)
        assert go(s, ("after", None)) == s                       # removing is always allowed
    for s in (UNDER["sets"], UNDER["clauses"]):
        assert go(s, ("after", "A2")) == s._replace(cursors="A2")
        assert go(s, ("after_from_results",)) == s._replace(cursors=M.FROM_RESULTS)


@pytest.mark.parametrize("client", M.CLIENTS)
def test_row_candidates_under_any_client(client):
    s = UNDER[client]
    assert M.step(s, ("candidates", "K"), NQ) == (s, M.ESTATE)
    assert M.step(s, ("bad_candidates",), NQ) == (s, M.ESTATE)
    assert go(s, ("candidates", None)) == s


@pytest.mark.parametrize("client", M.CLIENTS)
@pytest.mark.parametrize("call", [("upload", "Q2"), ("query", "short")])
def test_row_resident_set_replaced_drops_the_client(call, client):
    s = go(UNDER[client], call)
    assert M.expanded(s) is None and s.kind == "sets"
    assert (s.caps, s.cursors) == (None, None) and lists(s) == (None, None, None, "R")


def test_unknown_call():
    with pytest.raises(ValueError):
        M.step(M.initial(), ("nonsense",))
