"""The penalty rule of lmrs_batch_set_penalties (include/lmrs_hip.h) in numpy, literally: np.float32 scalars, one operation at a time.  The reference
of tests/test_batch_penalty.py; tests/test_batch_penalty_host.py holds it against a naive per-token loop."""
import numpy as np

NONE = 0xFFFFFFFF           # LMRS_TOKEN_NONE

# the parameter kinds of the tests: (repetition, presence, frequency, out_from); "freq" takes out_from = depth // 2 where it is used
KINDS = {
    "rep": dict(repetition=1.3),
    "boost": dict(presence=-1e4),
    "freq": dict(frequency=0.7, presence=0.2),
    "all": dict(repetition=1.7, presence=0.5, frequency=0.25, out_from=3),
    "sink": dict(frequency=1e4),
}


def params(kind, out_from=None):
    """the full parameter dict of a kind (None: no penalties)"""
    if kind is None:
        return None
    p = dict(repetition=1.0, presence=0.0, frequency=0.0, out_from=0)
    p.update(KINDS[kind])
    if out_from is not None:
        p["out_from"] = int(out_from)
    return p


def penalised(row, history, p, par):
    """row (float32 [V]) as the sinks see it for an output row at position p of a slot whose record is `history` (history[i] = the token at position i, NONE
    = unknown; only history[0 .. p] is read) under par = dict(repetition, presence, frequency, out_from), or None for no penalties"""
    out = np.asarray(row, np.float32).copy()
    if par is None:
        return out
    rep, pres, freq = np.float32(par["repetition"]), np.float32(par["presence"]), np.float32(par["frequency"])
    out_from = int(par["out_from"])
    c_all, c_out = {}, {}
    for i in range(p + 1):
        t = int(history[i])
        if t == NONE:
            continue
        c_all[t] = c_all.get(t, 0) + 1
        if i >= out_from:
            c_out[t] = c_out.get(t, 0) + 1
    with np.errstate(all="ignore"):
        if rep != np.float32(1.0):
            for t in c_all:
                l = out[t]
                out[t] = np.float32(l / rep) if l > np.float32(0.0) else np.float32(l * rep)
        for t, c in c_out.items():
            l = out[t]
            prod = np.float32(freq * np.float32(c))
            diff = np.float32(l - prod)
            out[t] = np.float32(diff - pres)
    return out
