"""Stress recipes: LMRS images whose activations leave the mild middle of every nonlinearity.

tools/synth_lmrs.py draws every weight from a narrow Gaussian, so a model built from it never underflows a softmax term, saturates a soft-cap,
quantises an all-zero group or ties two logits.  A recipe is a transform of the f32 master tensors (synth_lmrs.build_image(transform=...)) that
pushes ONE such regime into the model while every logit stays finite.  Each recipe has a witness among the oracle's regime counters
(oracle_lib.stats()); tests/test_stress_regimes.py asserts the witness on the CPU and then compares the HIP path with the oracle bit for bit.

The constants below were chosen by reading those counters on the CPU oracle (the values reached are recorded in DESIGN.md "Parity"), not guessed:
a recipe whose constant is softened makes its CPU witness test fail.

    image, cfg = build(cfg, recipe, q_type, seed)

Recipes: peaked, peaked_mild, softcap (Gemma), dead_groups, outliers, glu_extremes, tied_classifier, combined.
"""
from __future__ import annotations

import dataclasses
import warnings

import numpy as np

from tools import synth_lmrs as S

RECIPES = ("peaked", "peaked_mild", "softcap", "dead_groups", "outliers", "glu_extremes", "tied_classifier", "combined")

# q_proj and k_proj are both scaled, so attention scores grow with the SQUARE of these.  Stock scores spread over ~10 units.
#   peaked: spread of several hundred units - exp(score - max) is exactly 0 (argument below -103.98) for most keys, rows are one-hot.
#   peaked_mild: spread around a hundred - terms land between -87.34 and -103.98, where expf returns subnormals.
# Gemma-2 caps scores at +-50, so its softmax arguments never go below -100: exact zeros cannot occur there (exp(-100) = 3.8e-44 is a
# subnormal).  For Gemma `peaked` therefore witnesses subnormal terms and saturated caps, and the CPU test pins zeros == 0.
PEAKED_QK = {S.LLAMA: 8.0, S.PHI: 8.0, S.GEMMA: 16.0}
PEAKED_MILD_QK = {S.LLAMA: 4.0, S.PHI: 4.0, S.GEMMA: 7.0}
# softcap (Gemma): f32(tanh(s / 50)) is exactly 1 from s / 50 > 9.02 on - scores of several hundred; embed_tokens scaled until logits / 30 does the same
SOFTCAP_QK = 12.0
SOFTCAP_EMBED = 200.0
OUTLIER = 2.0e4
# SiLU: expf(-val) is +inf below val = -88.73; gate values are ~N(0, 0.03 * sqrt(dim)) per unit of normed input: scaled to a deviation of GLU_SIGMA
GLU_SIGMA = 150.0


def _block(n: int, k: int) -> slice:
    """the k-th 128-block of a vector of n, clamped to the last one"""
    b = min(k, n // 128 - 1)
    return slice(128 * b, 128 * b + 128)


def _narrow(cfg) -> float:
    """q and k values shrink with sqrt(dim) (rows of deviation 0.03 against a normed input): models narrower than the real ones get the difference back"""
    return max(1.0, float(np.sqrt(2048.0 / cfg.dim)))


def _peaked(table):
    def t(cfg, seed, name, layer, row0, w):
        return w * np.float32(table[cfg.model_type] * _narrow(cfg)) if name in ("q_proj", "k_proj") else w
    return t


def _softcap(cfg, seed, name, layer, row0, w):
    assert cfg.model_type == S.GEMMA, "softcap is a Gemma recipe"
    if name in ("q_proj", "k_proj"):
        return w * np.float32(SOFTCAP_QK * _narrow(cfg))
    if name == "embed_tokens":
        return w * np.float32(SOFTCAP_EMBED)
    return w


def _dead_groups(cfg, seed, name, layer, row0, w):
    gem = cfg.model_type == S.GEMMA
    dead = np.float32(-1.0 if gem else 0.0)                        # Gemma's kernels multiply by 1 + w (functional.rs:68-70)
    w = w.copy()
    if name == "input_layernorm":
        w[0, _block(cfg.dim, 0)] = dead                            # -> a zero group of x at the qkv quantiser
    elif name == "post_attention_layernorm" or (gem and name == "pre_feedforward_layernorm"):
        w[0, _block(cfg.dim, 1)] = dead                            # -> a zero group of xb2 at the w1/w3 quantiser (Gemma: the pre-ffn norm feeds it)
    elif name == "v_proj":
        # attention output dims 0..127 are zero when the V rows they are mixed from are: dim a of head a // hs reads kv row (head // kv_mul) * hs + a % hs
        kv_mul = cfg.n_heads // cfg.n_kv_heads
        a = np.arange(128)
        rows = np.unique((a // cfg.head_size // kv_mul) * cfg.head_size + a % cfg.head_size)
        w[rows[(rows >= row0) & (rows < row0 + w.shape[0])] - row0] = 0.0
    elif name == "gate_proj":
        b = _block(cfg.hidden_dim, 1)                              # act(0) * up = 0: a zero group of h at the w2 quantiser
        lo, hi = max(b.start, row0), min(b.stop, row0 + w.shape[0])
        if lo < hi:
            w[lo - row0:hi - row0] = 0.0
    return w


def _outlier_channels(cfg, seed, n, count):
    g = np.random.Generator(np.random.PCG64(np.random.SeedSequence([seed, 0x0171, n])))
    return np.sort(g.choice(n, size=count, replace=False))


def _outliers(cfg, seed, name, layer, row0, w):
    """A few residual channels OUTLIER times the rest: the columns of embed_tokens (the stream's start) and the rows of o_proj / down_proj that
    write those channels."""
    ch = _outlier_channels(cfg, seed, cfg.dim, 3)
    if name == "embed_tokens":
        w = w.copy(); w[:, ch] *= np.float32(OUTLIER)
    elif name in ("o_proj", "down_proj"):
        w = w.copy()
        rows = ch[(ch >= row0) & (ch < row0 + w.shape[0])] - row0
        w[rows] *= np.float32(OUTLIER)
    return w


def _glu_extremes(cfg, seed, name, layer, row0, w):
    if name == "gate_proj":
        return w * np.float32(GLU_SIGMA / (0.03 * np.sqrt(cfg.dim)))
    return w


def _tied_classifier(cfg, seed, name, layer, row0, w):
    """rows V/2 .. V of the classifier = rows 0 .. V/2: after quantisation every logit has a bit-identical twin V/2 rows away"""
    cls = "lm_head" if cfg.model_type == S.PHI else "embed_tokens"
    if name != cls:
        return w
    V, half = cfg.vocab_size, cfg.vocab_size // 2
    assert V % 2 == 0 and (V <= S.ROWS_PER_CHUNK or half % S.ROWS_PER_CHUNK == 0), "the twin rows must be whole slices"
    w = w.copy()
    if V <= S.ROWS_PER_CHUNK:
        w[half:] = w[:half]
    elif row0 >= half:
        fi = [f[0] for f in S.families(cfg)].index(cls)
        w[:] = S.float_tensor(cfg, seed, fi, 0, row0 - half, w.shape[0])
    return w


def _chain(*ts):
    def t(cfg, seed, name, layer, row0, w):
        for f in ts:
            w = f(cfg, seed, name, layer, row0, w)
        return w
    return t


TRANSFORMS = {
    "peaked": _peaked(PEAKED_QK),
    "peaked_mild": _peaked(PEAKED_MILD_QK),
    "softcap": _softcap,
    "dead_groups": _dead_groups,
    "outliers": _outliers,
    "glu_extremes": _glu_extremes,
    "tied_classifier": _tied_classifier,
    "combined": _chain(_peaked(PEAKED_MILD_QK), _outliers, _dead_groups),
}


def resolve(cfg, recipe: str) -> S.ModelCfg:
    """The geometry a recipe runs a config at.  Gemma's logit soft-cap covers the first `dim` logits only (transformer.rs:375), so a tied
    maximum needs both twins on the same side of it: tied_classifier runs Gemma with vocab_size == dim (every logit capped, the twin
    dim / 2 rows away)."""
    if isinstance(cfg, str):
        cfg = S.CONFIGS[cfg]
    if recipe == "tied_classifier" and cfg.model_type == S.GEMMA:
        cfg = dataclasses.replace(cfg, name=cfg.name + f"-v{cfg.dim}", vocab_size=cfg.dim)
    return cfg


def build(cfg, recipe: str, q_type: int = S.Q8_0, seed: int = 1234, threads: int | None = None):
    """-> (image, cfg): the LMRS image of `cfg` under `recipe`, a deterministic function of (cfg, recipe, q_type, seed)"""
    cfg = resolve(cfg, recipe)
    f = TRANSFORMS[recipe]
    with warnings.catch_warnings():
        # dead_groups zeroes whole weight rows: their groups quantise as 0 / 0 with scale 0, as they would in the reference's exporter (the
        # products with a zero scale are zero whatever the bytes)
        warnings.simplefilter("ignore", RuntimeWarning)
        img = S.build_image(cfg, q_type, seed=seed, threads=threads, transform=lambda name, layer, row0, w: f(cfg, seed, name, layer, row0, w))
    return img, cfg
