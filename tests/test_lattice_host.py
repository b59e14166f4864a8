"""Coverage by construction, on the host: the batched pass admits a LATTICE of geometries (prefill_batched_ok, lmrs_api.hip), and the kernel each GEMM of
a layer runs is chosen per launch from (n, o, tokens, format) by a cost model (gemm_q8_ring_tile, behind lmrs_debug_gemm_tile / gemm_tile: host
arithmetic, no GPU).  A CELL is what such a launch instantiates: (epilogue, tile rows x tile tokens, weight format, whether the row tile divides o).
This file sweeps the whole lattice for the cells it can reach and asserts that the corners of tools/synth_lmrs.py::lattice_corners, at the token
counts tests/test_lattice.py feeds them (FILL_TOKENS / SCORE_TOKENS below, imported there), together with the four mini shapes at the counts the
older tests feed those, reach every one of them.  Whether a corner is ADMITTED is not mirrored here: tests/test_lattice.py asserts it on the GPU."""
import collections
import functools
import itertools
import os

from tools import synth_lmrs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1024, 2048, 2304, 3072, 4096, 8192, 9216)           # rows_prologue_supported (lmrs_prefill.inc)
CHUNK = 512                                                   # kPrefillTokens: a longer run goes in passes of 512 tokens and a remainder
SWEEP_TOKENS = (48, 57, 100, 130, 300, 512) + tuple(range(513, 601))

Cell = collections.namedtuple("Cell", "epilogue tile_rows tile_tokens q4 ragged")

CORNERS = {c.name: c for c in S.lattice_corners()}
# fill_kv_cache token counts per corner: one in 48 .. 63, a ragged one between 64 and 200, one of 300 or more; beyond 512 (a 512-token pass, then 18
# tokens on the direct kernels) on two of the 1024-wide corners.  The wide corners stay at 300 tokens except those whose cell exists only higher up:
# wo / w2 of a 9216-wide model take 256 x 128 tiles, and the 2304 output rows of a 1024- or 2304-wide wo / w2 their 96 x 64 and 128 x 64 tiles, from 449
# tokens on (the two Gemma corners this sends to 512 tokens have 1024-wide attention and a narrow MLP: small models).
FILL_TOKENS = {name: (57, 130, 512) if c.dim == 1024 else (57, 130, 300) for name, c in CORNERS.items()}
FILL_TOKENS.update({"w1024-h1024": (57, 130, 300, 530), "w1024-h2304": (57, 130, 300, 512), "w1024-att9216": (57, 130, 300, 530),
                    "w9216-h1024": (57, 130, 460), "w2304-gqa3": (57, 130, 460), "gemma-att1024": (20, 57, 130, 512), "gemma-h2304": (57, 130, 512)})
# score_tokens / score_tokens_topk on every corner (the classifier launch); the corners with the vocabularies of 272 and of 4112 and one of 4096 at the
# lengths that move the classifier's tile (20: the direct kernels)
SCORE_TOKENS = {name: (60,) for name in CORNERS}
SCORE_TOKENS.update({"w1024-h1024": (20, 60), "w1024-h2304": (60, 100, 300, 512), "w1024-att3072": (20, 60, 300)})
# (config, format, tokens) of fill_kv_cache calls the suite already makes on the four mini shapes (test_gpu_parity.py::test_fill_kv_cache_batched_prefill,
# test_stress_regimes.py::test_fill_kv_cache_small_batch / _large_batch_...; mini-llama-long has mini-llama's shape)
MINI_FILLS = [("mini-llama", S.Q8_0, t) for t in (48, 70, 97, 200, 530, 600)] + [("mini-llama", S.Q4_0, t) for t in (70, 97)] + \
             [("mini-llama3b", S.Q8_0, t) for t in (33, 57, 83)] + [("mini-phi", S.Q8_0, t) for t in (63, 70, 140, 150)] + \
             [("mini-gemma", S.Q8_0, t) for t in (50, 61, 120)] + [("mini-gemma", S.Q4_0, t) for t in (61, 75)]
MINI_SCORES = [("mini-llama", S.Q8_0, 72), ("mini-llama", S.Q4_0, 72), ("mini-llama3b", S.Q8_0, 136), ("mini-phi", S.Q8_0, 136),
               ("mini-gemma", S.Q8_0, 72), ("mini-gemma", S.Q4_0, 72)]      # test_stress_regimes.py::test_token_entry_points (N_DECODE)
# classifier rows of the sweep: the vocabulary is no dimension of the lattice (a classifier of any row count is one EPI_STORE launch with row-major
# scales); the sweep takes the minis' 4096 rows and the corners' 272 and 4112 at every width
SWEEP_VOCABS = (272, 4096, 4112)

# Cells the sweep reaches and no corner can at a size this suite runs in seconds: (cell, the sentence that says why).  None.
UNREACHED = []


@functools.lru_cache(maxsize=None)
def _tile(n, o, n_tok, q4):
    import lmrs_amd
    return lmrs_amd.gemm_tile(n, o, n_tok, q4)[:2]


def passes(n_tok):
    """the token counts of the passes a run of n_tok tokens goes in"""
    return [min(CHUNK, n_tok - i) for i in range(0, n_tok, CHUNK)]


def _cell(epilogue, n, o, m, q4):
    tm, tn = _tile(n, o, m, q4)
    # below 48 tokens (0 x 0): the direct kernels, whose waves own 32 rows each
    return Cell(epilogue, tm, tn, bool(q4), o % (tm or 32) != 0)


def h_quantiser_fused(dim, hidden, m, q4):
    """test_stress_regimes.py::h_quantiser_fused (the mirror of gemm_q8_hq_fused) on plain numbers"""
    n, o = dim, 2 * hidden
    tm, tn = _tile(n, o, m, False)
    return not q4 and o % 256 == 0 and n % 256 == 0 and m >= 48 and tm >= 128 and tn == 128


def layer_cells(dim, att, kv, hidden, gemma, q4, n_tok):
    """the cells of a layer's four launches (prefill_layers, lmrs_api.hip: qkv | wo | w1/w3 | w2) over every pass of a run of n_tok tokens"""
    out = set()
    branch = "store" if gemma else "resid"                    # Gemma's branch outputs go to a buffer of their own; the others add to the residual stream
    for m in passes(n_tok):
        act = ("gelu" if gemma else "swiglu") + ("_q" if h_quantiser_fused(dim, hidden, m, q4) else "")
        out |= {_cell("qkv", dim, att + 2 * kv, m, q4), _cell(branch, att, dim, m, q4), _cell(act, dim, 2 * hidden, m, q4), _cell(branch, hidden, dim, m, q4)}
    return out


def classifier_cells(dim, vocab, q4, n_tok):
    """the classifier launch of the scoring pass (classify_rows): the written rows - the vocabulary less its last vocab % 4 - against every pass"""
    return {_cell("classifier", dim, vocab - vocab % 4, m, q4) for m in passes(n_tok)}


def cfg_layer_cells(c, q, n_tok):
    return layer_cells(c.dim, c.att_dim, c.kv_dim, c.hidden_dim, c.model_type == S.GEMMA, q == S.Q4_0, n_tok)


def corner_reach():
    """cell -> [(corner or mini, format, tokens, call)] in the order the lists above name them: the minis first"""
    reach = collections.OrderedDict()
    for name, q, t in MINI_FILLS:
        for x in cfg_layer_cells(S.CONFIGS[name], q, t):
            reach.setdefault(x, []).append((name, q, t, "fill"))
    for name, q, t in MINI_SCORES:
        c = S.CONFIGS[name]
        for x in cfg_layer_cells(c, q, t) | classifier_cells(c.dim, c.vocab_size, q == S.Q4_0, t):
            reach.setdefault(x, []).append((name, q, t, "score"))
    for name, c in CORNERS.items():
        for q in (S.Q8_0, S.Q4_0):
            for t in FILL_TOKENS[name]:
                for x in cfg_layer_cells(c, q, t):
                    reach.setdefault(x, []).append((name, q, t, "fill"))
            for t in SCORE_TOKENS[name]:
                for x in cfg_layer_cells(c, q, t) | classifier_cells(c.dim, c.vocab_size, q == S.Q4_0, t):
                    reach.setdefault(x, []).append((name, q, t, "score"))
    return reach


def lattice_sweep():
    """every cell the admitted lattice reaches at SWEEP_TOKENS -> {cell: one launch (n, o, tokens) that has it}.  The lattice is the seven widths cubed
    (dim, attention width, hidden) x the head sizes that divide the attention width (Gemma-2: dim 2304, 256) x kv heads in {1, 2, 4, 8, heads} x both
    formats; a cell belongs to ONE launch, so the sweep walks each launch's own factors: qkv (dim, attention width, head size, kv heads), wo (attention
    width, dim), w1/w3 (dim, hidden), w2 (hidden, dim), the classifier (dim, vocabulary)"""
    seen = {}

    def note(epilogue, n, o, gemma=False, hidden=0):
        for q4, t in itertools.product((False, True), SWEEP_TOKENS):
            for m in passes(t):
                e = epilogue + ("_q" if hidden and h_quantiser_fused(n, hidden, m, q4) else "")
                seen.setdefault(_cell(e, n, o, m, q4), (n, o, m))

    for dim, att in itertools.product(WIDTHS, WIDTHS):
        for hs in [h for h in (64, 96, 128) if att % h == 0] + ([256] if dim == 2304 and att % 256 == 0 else []):
            heads = att // hs
            for kvh in sorted({1, 2, 4, 8, heads}):
                if heads % kvh == 0:
                    note("qkv", dim, att + 2 * kvh * hs)
    for dim, other in itertools.product(WIDTHS, WIDTHS):          # other: the attention width (wo) or the hidden size (w2, w1/w3)
        note("resid", other, dim)
        note("swiglu", dim, 2 * other, hidden=other)
        if dim == 2304:
            note("store", other, dim)
            note("gelu", dim, 2 * other, hidden=other)
    for dim, vocab in itertools.product(WIDTHS, SWEEP_VOCABS):
        note("classifier", dim, vocab - vocab % 4)
    return seen


def coverage_table():
    """DESIGN.md section 4.4's table, one line per cell of the sweep: the first of the minis' and corners' calls that reaches it"""
    reach = corner_reach()
    lines = ["| epilogue | tile | format | row tile divides o | first reached by |", "|---|---|---|---|---|"]
    for x in sorted(lattice_sweep()):
        name, q, t, call = reach[x][0]
        tile = f"{x.tile_rows} x {x.tile_tokens}" if x.tile_rows else "direct"
        lines.append(f"| {x.epilogue} | {tile} | {'Q4_0' if x.q4 else 'Q8_0'} | {'no' if x.ragged else 'yes'} | {name} {'Q4_0' if q == S.Q4_0 else 'Q8_0'}, {call} of {t} |")
    return lines


def test_the_corners_stand_on_the_lattice_and_beside_the_configs():
    assert len(CORNERS) == len(S.lattice_corners()) and not set(CORNERS) & set(S.CONFIGS)
    shapes = {(c.dim, c.hidden_dim, c.n_heads, c.head_size, c.n_kv_heads, c.model_type) for c in S.CONFIGS.values()}
    for name, c in CORNERS.items():
        assert (c.dim, c.hidden_dim, c.n_heads, c.head_size, c.n_kv_heads, c.model_type) not in shapes, f"{name} repeats a shape of CONFIGS"
        assert c.n_layers == 2 and c.n_heads % c.n_kv_heads == 0
        assert (c.vocab_size - c.vocab_size % 4) % 16 == 0, f"{name}: a batch refuses classifiers whose written rows are no multiple of 16"
        assert c.model_type != S.GEMMA or c.vocab_size >= c.dim                    # the soft-cap loop indexes logits[0 .. dim)
        assert S.image_size(c, S.Q8_0) <= 210 << 20, f"{name}: {S.image_size(c, S.Q8_0) >> 20} MiB"
        fills = FILL_TOKENS[name]
        assert any(48 <= t <= 63 for t in fills) and any(64 < t < 200 and t % 64 for t in fills) and any(300 <= t <= 512 for t in fills)
        assert max(fills) + 8 + 2 <= c.max_pos, f"{name}: max_pos holds the longest fill behind 8 cached rows and two decode steps"
        assert max(fills) <= 512 or c.dim == 1024, "more than one pass on the narrow corners only"
    assert sum(max(t) > CHUNK for t in FILL_TOKENS.values()) >= 2
    assert {c.vocab_size for c in CORNERS.values()} >= {272, 4112}


def test_every_cell_of_the_lattice_is_reached_by_a_corner_or_a_mini():
    sweep, reach = lattice_sweep(), corner_reach()
    assert _tile.cache_info().currsize > 10000, "the sweep is the library's own host arithmetic, call by call"
    excused = {x for x, why in UNREACHED}
    assert all(isinstance(why, str) and len(why.split()) > 5 for x, why in UNREACHED) and excused <= set(sweep) and not excused & set(reach)
    missing = sorted(x for x in sweep if x not in reach and x not in excused)
    assert not missing, f"{len(missing)} of {len(sweep)} cells of the lattice are reached by no corner and no mini: " + \
        "; ".join(f"{x} (e.g. {sweep[x]})" for x in missing)
    # and the corners are what closes the gap: cells the minis alone leave out
    minis = {x for x, by in reach.items() if any(b[0] in S.CONFIGS for b in by)}
    new = set(sweep) - minis
    assert len(new) >= 15, sorted(new)
    assert {("resid", 256, 128), ("resid", 128, 128), ("qkv", 256, 128), ("swiglu", 32, 32), ("gelu", 64, 32)} <= {(x.epilogue, x.tile_rows, x.tile_tokens) for x in new}
    assert any(x.epilogue == "qkv" and x.ragged and x.tile_rows >= 128 for x in new), "a qkv row tile that straddles the q | k | v boundaries part-filled"


def test_the_design_document_carries_the_generated_table():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = "\n".join(coverage_table())
    assert table in text, "DESIGN.md section 4.4: regenerate the cell table with `PYTHONPATH=. python tests/test_lattice_host.py`"


if __name__ == "__main__":
    print("\n".join(coverage_table()))
