"""Parity on hostile activations.  Every other whole-model test runs on narrow Gaussian weights, which keep each nonlinearity in its mild
middle; here the models come from tests/stress_models.py, whose recipes push one numerical regime each into the forward pass - underflowing
and subnormal softmax terms, saturated soft-caps, all-zero quantisation groups, outlier channels, SiLU / GELU at their extremes, exactly tied
logits - with every logit finite.

CPU tier (unmarked): for every (recipe, family, format) the GPU tier uses, the oracle's regime counters (oracle_lib.stats()) witness that the
recipe reached its regime, and on tiny geometries the oracle is compared with the numpy transcription bit for bit in those regimes.
GPU tier: the HIP path against the oracle, bit for bit, on every decode form, the batched forward_layer, the token entry points, the
classifier's tie rule and the sampler.  The witnesses are asserted again there, on exactly the positions the comparison covers."""
import dataclasses
import functools

import numpy as np
import pytest

import numpy_ref as NR
import oracle_lib as O
import stress_models as SM
from parity_rules import assert_bit_equal, check_scores, ref_argmax
from tools import synth_lmrs as S

gpu = pytest.mark.gpu
SEED = 101

CASES = [("mini-llama", S.Q8_0), ("mini-llama", S.Q4_0), ("mini-llama3b", S.Q8_0), ("mini-phi", S.Q8_0), ("mini-gemma", S.Q8_0), ("mini-gemma", S.Q4_0)]
# positions of a decode run: across the merged launch's wave -> workgroup switch where the head size has one inside these configs' 256 positions
# (128 for the 96- and 128-wide heads; the 64-wide heads switch at 256 and Gemma's 256-wide have the workgroup form only: test_long_context_*)
N_DECODE = {"mini-llama": 72, "mini-llama3b": 136, "mini-phi": 136, "mini-gemma": 72}
N_CPU = 40                                       # the CPU tier runs the first positions of the same token sequence
ALL = ("peaked", "peaked_mild", "softcap", "dead_groups", "outliers", "glu_extremes", "tied_classifier", "combined")


def recipes_for(cfg, only=ALL):
    return [r for r in only if r != "softcap" or "gemma" in cfg]


MATRIX = [(c, q, r) for c, q in CASES for r in recipes_for(c)] + [("mini-llama", S.Q_NONE, "peaked"), ("mini-llama", S.Q_NONE, "glu_extremes")]


# ------------------------------------------------------------------ witnesses
def check_witness(recipe, cfg, q, st, rows, n_pos, decode=True):
    """The regime `recipe` exists for was reached: st = oracle_lib.stats() over the run, rows = its logits (every one finite)."""
    gem = cfg.model_type == S.GEMMA
    what = f"{cfg.name} q{q} {recipe} over {n_pos} positions: {st}"
    assert np.isfinite(rows).all(), f"{what}: a logit is not finite"
    if recipe == "peaked":
        if gem:
            # scores capped at +-50: softmax arguments stay above -100, where expf is subnormal but never 0 (stress_models.PEAKED_QK).
            # Single-token steps only: a batched forward_layer masks with its FIRST position (transformer.rs:525, `pos - t` on unsigned
            # integers wraps for the keys behind it), so its later rows carry -2.38e38 terms, whose exponentials are exact zeros.
            assert st["att_exp_subnormal"] > 0 and st["score_cap_sat"] > 0, what
            assert (st["att_exp_zero"] == 0) if decode else (st["att_exp_zero"] > 0), what
        else:
            assert st["att_exp_zero"] > 0, what
    if recipe in ("peaked_mild", "combined"):
        assert st["att_exp_subnormal"] > 0, what
    if recipe == "softcap":
        assert st["score_cap_sat"] > 0 and st["score_cap_bend"] > 0 and st["logit_cap_sat"] > 0, what
    if recipe in ("dead_groups", "combined") and q != S.Q_NONE:
        assert all(st["q_zero_" + s] > 0 for s in ("x", "att", "xb2", "h")), what
    if recipe in ("outliers", "combined") and q != S.Q_NONE:
        assert st["max_scale_ratio"] >= 1e4, what
    if recipe == "glu_extremes":
        if gem:      # stock weights already saturate a few hundred GELU calls in 40 steps; the recipe saturates nearly all of them
            assert st["gelu_tanh_sat"] > n_pos * cfg.n_layers * cfg.hidden_dim // 2, what
        else:
            assert st["silu_exp_inf"] > 0 and st["silu_arg_above_88"] > 0, what
    if recipe == "tied_classifier":
        ties = (rows == rows.max(axis=1, keepdims=True)).sum(axis=1)
        assert ties.min() >= 2, f"{what}: a step without a tied maximum ({ties.min()})"
        assert all(ref_argmax(r) < cfg.vocab_size // 2 for r in rows), f"{what}: the reference's rule must pick the lower twin"


@functools.lru_cache(maxsize=None)
def image_of(cfg, q, recipe):
    return SM.build(cfg, recipe, q, SEED)


@functools.lru_cache(maxsize=None)
def oracle_decode(cfg, q, recipe, n):
    """n sequential forwards of the oracle from position 0 -> (image, cfg, tokens, logits [n, V], {(which, layer, pos): K/V row}, stats)"""
    img, c = image_of(cfg, q, recipe)
    toks = S.prompt_tokens(c, n, SEED)
    orc = O.Oracle(img)
    O.stats_reset()
    rows = np.stack([orc.forward(int(t), pos).copy() for pos, t in enumerate(toks)])
    st = O.stats()
    kv = {(w, l, p): orc.kv_row(w, l, p) for w in (0, 1) for l in range(c.n_layers) for p in (0, n // 2, n - 1)}
    return img, c, toks, rows, kv, st


# ------------------------------------------------------------------ CPU tier
@pytest.mark.parametrize("cfg,q,recipe", MATRIX)
def test_recipe_reaches_its_regime(cfg, q, recipe):
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, recipe, N_CPU)
    print(f"\n{c.name} q{q} {recipe}: {({k: v for k, v in st.items() if v})}")
    check_witness(recipe, c, q, st, rows, N_CPU)


def test_stock_weights_reach_none_of_the_regimes():
    """What the recipes are for: the same counters on the stock image stay at zero (Gemma's GELU saturates a few hundred times)."""
    for cfg in ("mini-llama", "mini-gemma"):
        orc = O.Oracle(S.build_image(cfg, S.Q8_0, seed=SEED))
        O.stats_reset()
        for pos, t in enumerate(S.prompt_tokens(cfg, N_CPU, SEED)):
            orc.forward(int(t), pos)
        st = O.stats()
        assert st.pop("max_scale_ratio") < 100 and st.pop("gelu_tanh_sat") < 1000
        bend = st.pop("score_cap_bend")            # Gemma's stock scores reach the cap's bend now and then; Llama has no cap at all
        assert bend == 0 or cfg == "mini-gemma", bend
        assert not any(st.values()), st


def test_witnesses_do_not_depend_on_the_thread_count():
    """The integer counters are atomic: one thread and the default team count the same (attention runs under OpenMP)."""
    img, c = image_of("mini-llama", S.Q8_0, "peaked")
    toks = S.prompt_tokens(c, 12, SEED)
    got = []
    n0 = O.threads()
    for n in (1, max(n0, 4)):                     # (a team of at least four whatever the environment's default)
        O.set_threads(n)
        orc = O.Oracle(img); O.stats_reset()
        lg = [orc.forward(int(t), pos).copy() for pos, t in enumerate(toks)]
        got.append((O.stats(), np.stack(lg)))
    O.set_threads(n0)
    assert got[0][0] == got[1][0]
    assert_bit_equal(got[0][1], got[1][1], "logits, 1 thread vs the team")


@pytest.mark.parametrize("cfg,q", [("tiny-llama", S.Q8_0), ("tiny-gemma", S.Q4_0), ("tiny-phi", S.Q_NONE), ("mini-llama", S.Q8_0)])
def test_identity_transform_leaves_the_image_bytes_unchanged(cfg, q):
    assert np.array_equal(S.build_image(cfg, q, seed=3, transform=lambda name, layer, row0, w: w), S.build_image(cfg, q, seed=3))


def tiny_cfg(cfg, recipe):
    """dead_groups on a 128-wide model would zero its ONE group of x and of xb2, i.e. switch attention and the FFN off: there the tiny
    geometries run at dim 256 / hidden 512 with at least 256 attention dims, so that every quantised vector keeps a live group."""
    c = S.CONFIGS[cfg]
    if recipe == "dead_groups":
        c = dataclasses.replace(c, name=c.name + "-d256", dim=256, hidden_dim=512)
        if c.att_dim < 256:
            c = dataclasses.replace(c, n_heads=2 * c.n_heads, n_kv_heads=2 * c.n_kv_heads)
    return c


@pytest.mark.parametrize("cfg", ["tiny-llama", "tiny-gemma", "tiny-phi"])
@pytest.mark.parametrize("q", [S.Q8_0, S.Q4_0])
@pytest.mark.parametrize("recipe", ["peaked", "dead_groups", "glu_extremes"])
def test_oracle_matches_numpy_transcription_in_the_regime(cfg, q, recipe):
    """The oracle judges the GPU alone, and its transcription check (test_oracle_vs_numpy.py) only ever saw Gaussians: the two transcriptions
    of the Rust sources again, on the recipes, logits bit for bit - with the witness that the tiny model reached the regime too."""
    img, c = image_of(tiny_cfg(cfg, recipe), q, recipe)
    orc = O.Oracle(img); ref = NR.NumpyModel(img)
    toks = S.prompt_tokens(c, 16, SEED)
    O.stats_reset()
    rows = []
    for pos, t in enumerate(toks):
        lo = orc.forward(int(t), pos).copy(); ln = ref.forward(int(t), pos)
        assert_bit_equal(lo, ln, f"{cfg} q{q} {recipe} pos {pos}")
        rows.append(lo)
    check_witness(recipe, c, q, O.stats(), np.stack(rows), len(toks))


# ------------------------------------------------------------------ GPU tier
@pytest.fixture(scope="module")
def L():
    import lmrs_amd
    return lmrs_amd


def check_kv(m, kv, what):
    for (w, l, p), row in kv.items():
        assert_bit_equal(m.kv_row(w, l, p), row, f"{what}: {'key' if w == 0 else 'value'} row, layer {l}, pos {p}")


FORMS = {"merged": {}, "separate": {"LMRS_QKV_ATT": "0"}, "split": {"LMRS_ATT_SPLIT_POS": "16"}}


def decode_and_compare(L, monkeypatch, cfg, q, recipe, n, env):
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, recipe, n)
    check_witness(recipe, c, q, st, rows, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = L.Transformer(img)
    what = f"{c.name} q{q} {recipe} {env}"
    for pos, t in enumerate(toks):
        assert_bit_equal(m.forward(int(t), pos), rows[pos], f"{what}: logits at pos {pos}")
    check_kv(m, kv, what)
    m.close()


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("cfg,q,recipe", MATRIX)
def test_decode_forms(L, monkeypatch, cfg, q, recipe, form):
    """forward at every position: the merged qkv + attention launch in the forms the run crosses, the separate kernels (LMRS_QKV_ATT=0), the
    split attention from position 16 on - logits at every position, K/V rows of every layer at the first / middle / last position."""
    decode_and_compare(L, monkeypatch, cfg, q, recipe, N_DECODE[cfg], FORMS[form])


@gpu
@pytest.mark.parametrize("env", [{}, {"LMRS_QKV_ATT": "0"}, {"LMRS_ATT_SPLIT_POS": "40"}, {"LMRS_ATT_SPLIT_POS": "0"}], ids=["default", "separate", "split40", "nosplit"])
def test_decode_forms_on_a_long_context(L, monkeypatch, env):
    """1100 positions of mini-llama-long on peaked rows.  By default: the wave form of the merged launch to 255, its workgroup form to 383, then the
    split attention in its buckets below and above 1024 keys; LMRS_ATT_SPLIT_POS=40: the split pair nearly throughout; =0 (never split): the
    workgroup form up to qa_max_T = 1024 and the separate kernels past it."""
    decode_and_compare(L, monkeypatch, "mini-llama-long", S.Q8_0, "peaked", 1100, env)


# the 64-wide heads leave the wave form of the merged launch at position 256 - beyond mini-llama's 256 positions: every recipe again on
# mini-llama-long, both formats, 300 positions (wave form to 255, workgroup form from 256 on)
LONG64 = [(q, r) for q in (S.Q8_0, S.Q4_0) for r in recipes_for("mini-llama-long")]


@gpu
@pytest.mark.parametrize("q,recipe", LONG64)
def test_decode_crosses_the_wave_and_workgroup_forms_at_head_size_64(L, monkeypatch, q, recipe):
    decode_and_compare(L, monkeypatch, "mini-llama-long", q, recipe, 300, {})


def h_quantiser_fused(L, c, n_tok):
    """The batched w1/w3 launch of n_tok tokens takes the epilogue that quantises h.  A mirror of gemm_q8_hq_fused (lmrs_prefill.inc), term for
    term, over the tile the library itself reports (lmrs_debug_gemm_tile): keep the two in step."""
    n, o = c.dim, 2 * c.hidden_dim
    tm, tn, _ = L.gemm_tile(n, o, n_tok, False)
    return o % 256 == 0 and n % 256 == 0 and n_tok >= 48 and tm >= 128 and tn == 128


@functools.lru_cache(maxsize=None)
def oracle_fill(cfg, q, recipe, pos0, n_tok):
    img, c = image_of(cfg, q, recipe)
    orc = O.Oracle(img)
    O.stats_reset()
    if pos0:
        b0 = orc.get_embeddings(S.prompt_tokens(c, pos0, SEED + 1))
        assert orc.fill_kv_cache(b0, 0) == pos0
    b = orc.get_embeddings(S.prompt_tokens(c, n_tok, SEED + 2))
    assert orc.fill_kv_cache(b, pos0) == pos0 + n_tok
    kv = {(w, l, p): orc.kv_row(w, l, p) for w in (0, 1) for l in range(c.n_layers) for p in (pos0, pos0 + n_tok // 2, pos0 + n_tok - 1)}
    steps, t = [], 7
    for pos in range(pos0 + n_tok, pos0 + n_tok + 2):
        lo = orc.forward(t, pos).copy()
        steps.append((t, pos, lo)); t = ref_argmax(lo)
    st = O.stats()
    assert np.isfinite(b).all()
    return img, c, b, kv, steps, st


def fill_and_compare(L, cfg, q, recipe, pos0, n_tok, fused):
    img, c, b, kv, steps, st = oracle_fill(cfg, q, recipe, pos0, n_tok)
    check_witness(recipe, c, q, st, np.stack([s[2] for s in steps]), n_tok + 2, decode=False)
    assert h_quantiser_fused(L, c, n_tok) == (fused and q == S.Q8_0), f"{n_tok} tokens of {c.name}: the w1/w3 launch is not the one this test is for"
    m = L.Transformer(img)
    if pos0:
        a0 = m.get_embeddings(S.prompt_tokens(c, pos0, SEED + 1))
        assert m.fill_kv_cache(a0, 0) == pos0
    a = m.get_embeddings(S.prompt_tokens(c, n_tok, SEED + 2))
    assert m.fill_kv_cache(a, pos0) == pos0 + n_tok
    what = f"{c.name} q{q} {recipe}, {n_tok} tokens at {pos0}"
    assert_bit_equal(a, b, f"{what}: residual stream after the batched layers")
    check_kv(m, kv, what)
    for t, pos, lo in steps:
        assert_bit_equal(m.forward(t, pos), lo, f"{what}: decode at {pos} on the prefilled cache")
    m.close()


SMALL_BATCH = {"mini-llama": 97, "mini-llama3b": 83, "mini-phi": 70, "mini-gemma": 61}     # ragged; below the token count from which w1/w3 quantises h itself
FILL_RECIPES = ("peaked", "peaked_mild", "softcap", "dead_groups", "outliers", "glu_extremes", "combined")
# scores: in LDS (default), memory-resident, and - where the switch exists, Gemma-2's block attention - the long-batch forms
FILL_MATRIX = [(c, q, r, s) for c, q in CASES for r in recipes_for(c, FILL_RECIPES) for s in ("lds", "memory") + (("long_forms",) if "gemma" in c else ())]
FILL_MATRIX += [("mini-llama", S.Q_NONE, r, "lds") for r in ("peaked", "glu_extremes")]       # f32 weights: fill_kv_cache over lmrs_f32.inc


@gpu
@pytest.mark.parametrize("cfg,q,recipe,scores", FILL_MATRIX)
def test_fill_kv_cache_small_batch(L, monkeypatch, cfg, q, recipe, scores):
    """forward_layer over a ragged token batch behind 7 cached positions: block attention with its scores in LDS, memory-resident
    (LMRS_ATT_LDS_KEYS=32) and, Gemma-2, in its long-batch forms - residual stream, K/V rows, two decode steps on that cache."""
    if scores == "memory": monkeypatch.setenv("LMRS_ATT_LDS_KEYS", "32")
    if scores == "long_forms": monkeypatch.setenv("LMRS_ATT_LONG_BATCH_FORMS", "1")
    fill_and_compare(L, cfg, q, recipe, 7, SMALL_BATCH[cfg], fused=False)


@gpu
@pytest.mark.parametrize("cfg,n_tok", [("mini-llama", 200), ("mini-phi", 150), ("mini-gemma", 120)])
@pytest.mark.parametrize("recipe", ["dead_groups", "outliers", "glu_extremes"])
def test_fill_kv_cache_large_batch_quantises_h_in_the_w13_epilogue(L, cfg, recipe, n_tok):
    """A batch large enough for the w1/w3 GEMM to apply the activation and quantise h in its epilogue (asserted through the library's own
    tile rule): zero groups of h, outlier scales and saturated activations in the fused copy of the quantiser."""
    fill_and_compare(L, cfg, S.Q8_0, recipe, 0, n_tok, fused=True)


TOKEN_RECIPES = ("peaked", "peaked_mild", "softcap", "tied_classifier")
TOKEN_MATRIX = [(c, q, r) for c, q in CASES for r in recipes_for(c, TOKEN_RECIPES)] + [("mini-llama", S.Q_NONE, "peaked")]


@gpu
@pytest.mark.parametrize("cfg,q,recipe", TOKEN_MATRIX)
def test_token_entry_points(L, cfg, q, recipe):
    """forward_tokens, score_tokens and prefill_tokens over the decode run's tokens as ONE batched pass (asserted: lmrs_tokens_path, Gemma-2
    included): logits of every position bit for bit, log-probabilities by parity_rules.py's rule, K/V rows and the forward that follows."""
    n = N_DECODE[cfg]
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, recipe, n)
    check_witness(recipe, c, q, st, rows, n)
    what = f"{c.name} q{q} {recipe}"
    m = L.Transformer(img)
    # every quantised model, Gemma-2 included, takes the batched pass; f32 weights go token by token over lmrs_f32.inc
    assert m.tokens_path(n - 1) is (q != S.Q_NONE), f"{what}: the token run took the wrong path"
    assert_bit_equal(m.forward_tokens(toks[:n - 1], 0), rows[:n - 1], f"{what}: forward_tokens, logits of every position")
    assert_bit_equal(m.forward(int(toks[n - 1]), n - 1), rows[n - 1], f"{what}: forward after forward_tokens")
    check_kv(m, kv, what + " forward_tokens")
    m2 = L.Transformer(img)
    check_scores(m2.score(toks, 0), rows, toks, what)
    check_kv(m2, kv, what + " score")
    m3 = L.Transformer(img)
    assert m3.prefill_tokens(toks[:n - 1], 0) == n - 1
    assert_bit_equal(m3.forward(int(toks[n - 1]), n - 1), rows[n - 1], f"{what}: forward after prefill_tokens")
    check_kv(m3, kv, what + " prefill_tokens")
    for x in (m, m2, m3): x.close()


@gpu
@pytest.mark.parametrize("cfg,q,recipe", [("mini-llama", S.Q8_0, "peaked"), ("mini-gemma", S.Q8_0, "softcap"), ("mini-phi", S.Q8_0, "tied_classifier")])
def test_token_entry_points_agree_with_the_token_by_token_path(L, monkeypatch, cfg, q, recipe):
    n = N_DECODE[cfg]
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, recipe, n)
    a = L.Transformer(img)
    monkeypatch.setenv("LMRS_NO_BATCHED_PREFILL", "1")
    b = L.Transformer(img)
    monkeypatch.delenv("LMRS_NO_BATCHED_PREFILL")
    assert a.tokens_path(n) and not b.tokens_path(n)
    ra, rb = a.score(toks, 0), b.score(toks, 0)
    assert_bit_equal(ra[0], rb[0], "log-probabilities, batched vs token by token")
    assert ra[1].tolist() == rb[1].tolist() and ra[2] == rb[2]
    check_scores(ra, rows, toks, f"{c.name} {recipe}")
    assert_bit_equal(b.forward_tokens(toks, 0), rows, f"{c.name} {recipe}: forward_tokens token by token")
    a.close(); b.close()


@gpu
@pytest.mark.parametrize("cls_tail", ["1", "0"])
@pytest.mark.parametrize("cfg,q", CASES)
def test_tied_classifier_first_maximum_wins(L, monkeypatch, cfg, q, cls_tail):
    """Every logit has a bit-identical twin V/2 rows away, in another classifier workgroup: forward_argmax at every position and 48 greedy
    tokens (the multi-step graphs; the argmax folded into the classifier's tail, and as a launch of its own with LMRS_CLS_TAIL=0) must pick
    the lower index, as sample_argmax's strict `>` does (sampler.rs:29-41)."""
    n = N_DECODE[cfg]
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, "tied_classifier", n)
    check_witness("tied_classifier", c, q, st, rows, n)
    monkeypatch.setenv("LMRS_CLS_TAIL", cls_tail)
    m = L.Transformer(img)
    for pos, t in enumerate(toks):
        want = ref_argmax(rows[pos])
        got = m.forward_argmax(int(t), pos)
        assert got == want and got < c.vocab_size // 2, f"{c.name} q{q} pos {pos}: device {got}, reference {want}"
    prompt = toks[:6]
    m2 = L.Transformer(img)
    got = m2.generate_greedy(prompt, 48)
    m2.close()
    ref = O.Oracle(img).generate_greedy(prompt, 48)
    assert (got == ref).all(), f"first mismatch at {int(np.flatnonzero(got != ref)[0])}: {got} vs {ref}"
    assert (ref < c.vocab_size // 2).all()
    m.close()


@gpu
@pytest.mark.parametrize("cfg,q,world,plan", [("mini-llama", S.Q8_0, 2, "cls"), ("mini-llama", S.Q8_0, 2, "tp"), ("mini-llama", S.Q8_0, 8, "cls"),
                                              ("mini-gemma", S.Q8_0, 2, "cls"), ("mini-phi", S.Q8_0, 2, "tp")])
def test_tied_classifier_across_row_shards(L, monkeypatch, cfg, q, world, plan):
    """The twins V/2 rows apart live on different shards (with 8 shards: four shards apart): the merge of the shards' argmax partials must
    keep the lower index.  Logits bit for bit as well."""
    monkeypatch.setenv("LMRS_SHARD_PLAN", plan)
    img, c, toks, rows, kv, st = oracle_decode(cfg, q, "tied_classifier", N_DECODE[cfg])
    grp = L.ShardGroup(img, world)
    for pos in range(16):
        lg, nxt = grp.forward(int(toks[pos]), pos)
        assert_bit_equal(lg, rows[pos], f"{c.name} world={world} {plan}: logits at pos {pos}")
        assert nxt == ref_argmax(rows[pos]) and nxt < c.vocab_size // 2
    grp.close()


@gpu
@pytest.mark.parametrize("cfg,q,recipe", [("mini-llama", S.Q8_0, "peaked"), ("mini-phi", S.Q8_0, "peaked_mild"), ("mini-gemma", S.Q8_0, "peaked"),
                                          ("mini-gemma", S.Q8_0, "softcap"), ("mini-gemma", S.Q4_0, "softcap")])
def test_sampler_on_stress_logits(L, cfg, q, recipe):
    """forward_sample with temperature and top-p against the oracle's forward + the oracle's sampler, 30 steps each: softcap's logits reach
    thousands (the softmax over them is one-hot after the temperature), peaked ones stay small."""
    img, c = image_of(cfg, q, recipe)
    prompt = S.prompt_tokens(c, 4, SEED)
    for temperature, top_p in [(0.7, 0.9), (1.3, 0.5), (0.9, 1.0)]:
        a = L.Transformer(img); o = O.Oracle(img)
        V = c.vocab_size
        sa = L.Sampler(V, temperature, top_p, 4242); so = O.Sampler(V, temperature, top_p, 4242)
        to = None
        for pos in range(30):
            t = int(prompt[pos]) if pos < len(prompt) else to
            ta = a.forward_sample(t, pos, sa)
            to = so.sample(o.forward(t, pos).copy())
            assert ta == to, f"{c.name} q{q} {recipe} temperature {temperature} top_p {top_p} pos {pos}: device {ta}, oracle {to}"
        a.close()
