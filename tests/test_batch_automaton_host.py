"""The token automaton's host side (include/lmrs_hip.h: lmrs_automaton_check, lmrs_automaton_walk) and the two builders of lmrs_amd.TokenAutomaton:
plain arithmetic, judged against numpy and Python loops.  No GPU."""
import numpy as np
import pytest

import lmrs_amd as L

DEAD = L.STATE_DEAD


def random_tables(rng, V, n_states, n_classes, p_dead=0.5):
    class_of = rng.integers(0, n_classes, V).astype(np.uint16)
    nxt = rng.integers(0, n_states, (n_states, n_classes)).astype(np.uint32)
    dead = rng.random((n_states, n_classes)) < p_dead
    nxt[dead] = DEAD
    return class_of, nxt


def test_the_header_names_what_python_names():
    assert (L.STATE_DEAD, L.FINISH_FINAL, L.AUTOMATA_MAX) == (0xFFFFFFFF, 3, 16)
    for name in ("lmrs_automaton_check", "lmrs_automaton_walk", "lmrs_batch_automaton_create", "lmrs_batch_automaton_destroy", "lmrs_batch_attach_automaton",
                 "lmrs_batch_automaton_state", "lmrs_batch_automaton_advance", "lmrs_op_automaton_masks"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)


def test_the_cpp_example_and_host_mirror_compile():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", os.path.join(root, "lm.rs_amd", "hostcpp", "batch_grammar.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hpp = open(os.path.join(root, "lm.rs_amd", "hostcpp", "transformer.hpp")).read()
    for name in ("lmrs_batch_automaton_create", "lmrs_batch_automaton_destroy", "lmrs_batch_attach_automaton", "lmrs_batch_automaton_state", "lmrs_batch_automaton_advance",
                 "LMRS_FINISH_FINAL", "LMRS_STATE_DEAD"):
        assert name in hpp, name


def test_check_messages_one_per_rule():
    ok = L.TokenAutomaton([0, 1, 1, 0], [[1, DEAD], [DEAD, 0]])
    assert ok.check().tolist() == [2, 2]
    cases = [
        # a class at or above n_classes: the token and the class
        (L.TokenAutomaton([0, 1, 2, 0], [[1, DEAD], [DEAD, 0]]), "token 2: class 2 is not below n_classes = 2"),
        # a next entry that is neither a state nor DEAD: the state and the class
        (L.TokenAutomaton([0, 1, 1, 0], [[1, DEAD], [DEAD, 2]]), "state 1, class 1: next = 2 is neither a state below n_states = 2 nor LMRS_STATE_DEAD"),
        # a state that is not final and allows nothing
        (L.TokenAutomaton([0, 1, 1, 0], [[1, DEAD], [DEAD, DEAD]]), "state 1 is not final and every class of it is dead"),
        # its only live class holds no token
        (L.TokenAutomaton([0, 0, 0, 0], [[1, DEAD], [DEAD, 0]]), "state 1 is not final and its live classes hold no token below vocab_size = 4 (class 1 is empty)"),
    ]
    for ta, msg in cases:
        with pytest.raises(L.LmrsError) as e:
            ta.check()
        assert str(e.value).startswith("lmrs_automaton_check: " + msg), (msg, str(e.value))
    # the same two states are fine once they are final, and count 0
    assert L.TokenAutomaton([0, 1, 1, 0], [[1, DEAD], [DEAD, DEAD]], final=[0, 1]).check().tolist() == [2, 0]
    assert L.TokenAutomaton([0, 0, 0, 0], [[1, DEAD], [DEAD, 0]], final=[0, 1]).check().tolist() == [4, 0]
    # the sizes
    lib, z = L.lib(), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data
    c16 = np.zeros(4, np.uint16)
    for args, msg in [((4, 0, 1), "n_states = 0 is outside"), ((4, 1 << 31, 1), "n_states = 2147483648 is outside"), ((4, 1, 0), "n_classes = 0 is outside"),
                      ((4, 1, 65537), "n_classes = 65537 is outside"), ((0, 1, 1), "vocab_size is 0")]:
        assert lib.lmrs_automaton_check(*args, p(c16), p(z), None, None) != 0
        assert lib.lmrs_last_error().decode().startswith("lmrs_automaton_check: " + msg), msg
    assert lib.lmrs_automaton_check(4, 1, 1, None, p(z), None, None) != 0 and lib.lmrs_last_error().decode().startswith("lmrs_automaton_check: NULL argument")


@pytest.mark.parametrize("V,n_states,n_classes", [(33, 1, 1), (2052, 3, 2), (4096, 70, 300), (500, 5, 65536)])
def test_n_allowed_against_a_numpy_count(V, n_states, n_classes):
    rng = np.random.default_rng(V + n_states)
    class_of, nxt = random_tables(rng, V, n_states, n_classes)
    ta = L.TokenAutomaton(class_of, nxt, final=np.ones(n_states, bool))          # (all final: a state may allow nothing)
    want = [(nxt[q][class_of] != DEAD).sum() for q in range(n_states)]
    assert ta.check().tolist() == want
    assert [int(ta.allowed(q).sum()) for q in range(n_states)] == want


def test_walk_against_a_python_loop():
    rng = np.random.default_rng(5)
    V = 300
    class_of, nxt = random_tables(rng, V, 9, 6, p_dead=0.25)
    ta = L.TokenAutomaton(class_of, nxt, final=np.ones(9, bool))
    stopped = complete = 0
    for trial in range(200):
        toks = rng.integers(0, V, int(rng.integers(0, 12)))
        q0 = int(rng.integers(0, 9))
        q, k, ok = q0, 0, True
        for t in toks:
            nx = int(nxt[q, class_of[t]])
            if nx == DEAD:
                ok = False
                break
            q, k = nx, k + 1
        assert ta.walk(q0, toks) == (q, k, ok), (trial, q0, toks.tolist())
        stopped += not ok; complete += ok
    assert stopped >= 20 and complete >= 20
    # the message of a stop names the token and the state in front of it
    t_dead = next(t for t in range(V) if nxt[0, class_of[t]] == DEAD)
    assert ta.walk(0, [t_dead]) == (0, 0, False)
    assert L.lib().lmrs_last_error().decode() == f"lmrs_automaton_walk: token 0 = {t_dead} is not allowed in state 0 (0 tokens walked)"
    # arguments out of range raise
    with pytest.raises(L.LmrsError, match=r"^lmrs_automaton_walk: state 9 of 9"):
        ta.walk(9, [1])
    with pytest.raises(L.LmrsError, match=r"^lmrs_automaton_walk: token 1 = 300 is not below vocab_size = 300"):
        ta.walk(0, [next(t for t in range(V) if nxt[0, class_of[t]] != DEAD), 300])


def test_from_transitions_against_the_dense_table():
    rng = np.random.default_rng(6)
    V, n_states = 700, 6
    # few distinct columns: every token copies one of 11 prototype columns
    proto = rng.integers(0, n_states, (n_states, 11)).astype(np.uint32)
    proto[rng.random(proto.shape) < 0.4] = DEAD
    proto[:, 0] = np.arange(n_states)[::-1]                                     # (one column without a dead entry: every state allows something)
    dense = proto[:, rng.integers(0, 11, V)]
    dense[:, 3] = proto[:, 0]
    ta = L.TokenAutomaton.from_transitions(V, dense)
    assert ta.n_classes <= 11 and ta.n_states == n_states and ta.vocab_size == V
    ta.check()
    for q in range(n_states):
        assert np.array_equal(ta.next[q][ta.class_of], dense[q]), f"state {q}: successors and allowed sets"
        assert np.array_equal(ta.allowed(q), dense[q] != DEAD)
    # the dict form gives the same automaton
    rows = [{t: int(dense[q, t]) for t in range(V) if dense[q, t] != DEAD} for q in range(n_states)]
    tb = L.TokenAutomaton.from_transitions(V, rows)
    assert all(np.array_equal(tb.next[q][tb.class_of], dense[q]) for q in range(n_states))


def test_from_sequences_on_labels_that_share_prefixes():
    V = 100
    labels = [[7], [20, 21], [20, 22, 23], [20, 22, 24]]
    ta = L.TokenAutomaton.from_sequences(V, labels)
    n_allowed = ta.check()
    assert ta.allowed(0).nonzero()[0].tolist() == [7, 20]
    for lab in labels:
        q, k, ok = ta.walk(0, lab)
        assert ok and k == len(lab) and ta.final[q] and n_allowed[q] == 0, lab
        for cut in range(1, len(lab)):
            q, k, ok = ta.walk(0, lab[:cut])
            assert ok and not ta.final[q] and n_allowed[q] >= 1
    q, _, _ = ta.walk(0, [20])
    assert ta.allowed(q).nonzero()[0].tolist() == [21, 22]
    q, _, _ = ta.walk(0, [20, 22])
    assert ta.allowed(q).nonzero()[0].tolist() == [23, 24]
    assert ta.walk(0, [20, 23]) == (ta.walk(0, [20])[0], 1, False)
    assert ta.n_states == 1 + 1 + 2 + 3 and int(ta.final.sum()) == 4
    for bad in ([[5], []], [[5], [5, 6]], [[5, 6], [5]], [[100]]):
        with pytest.raises(L.LmrsError, match="from_sequences"):
            L.TokenAutomaton.from_sequences(V, bad)
