"""lm.rs_amd — MI355X-native decode hot path for lm.rs models (host-side mirror, Python flavour).

`Transformer` mirrors the public surface of `lmrs::transformer::Transformer`
(reference src/transformer.rs:127-131, :134, :316, :659, :672) over the C ABI of
`liblmrs_hip.so` (include/lmrs_hip.h).  There is NO CPU fallback: if the HIP library is
missing or no GPU is visible, construction raises.

The directory name contains a dot, so import it through the repo-root shim:  `import lmrs_amd`.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblmrs_hip.so")
CSRC = os.path.join(_HERE, "csrc")

GEMMA, LLAMA, PHI = 0, 1, 2
Q_NONE, Q8_0, Q4_0 = 0, 1, 2

# every symbol include/lmrs_hip.h declares (tests/test_abi.py checks the header against this list)
EXPORTS = [
    "lmrs_create", "lmrs_create_sharded", "lmrs_comm_unique_id", "lmrs_destroy", "lmrs_get_args", "lmrs_forward",
    "lmrs_forward_argmax", "lmrs_get_embeddings", "lmrs_fill_kv_cache", "lmrs_generate_greedy", "lmrs_forward_tokens", "lmrs_score_tokens",
    "lmrs_prefill_tokens", "lmrs_tokens_path", "lmrs_score_tokens_topk", "lmrs_forward_topk", "lmrs_op_topk",
    "lmrs_verify_tokens", "lmrs_draft_lookup", "lmrs_generate_speculative", "lmrs_debug_gemm_skinny",
    "lmrs_batch_create", "lmrs_batch_destroy", "lmrs_batch_prefill", "lmrs_batch_fork", "lmrs_batch_forward", "lmrs_batch_generate_greedy",
    "lmrs_batch_debug_kv", "lmrs_batch_forward_runs", "lmrs_batch_forward_sample", "lmrs_batch_create_wide", "lmrs_batch_width", "lmrs_debug_gemm_wide", "lmrs_op_sample_rows", "lmrs_sampler_topp_sorted_pairs", "lmrs_bench_sample_rows",
    "lmrs_batch_forward_runs_sample", "lmrs_op_sort_candidates",
    "lmrs_batch_prefill_embeddings", "lmrs_batch_forward_runs_embed", "lmrs_batch_forward_runs_embed_sample",
    "lmrs_batch_create_paged", "lmrs_batch_pages", "lmrs_batch_slot_pages", "lmrs_batch_release", "lmrs_batch_prefill_form", "lmrs_batch_debug_prefill_table",
    "lmrs_batch_set_masks", "lmrs_batch_clear_masks", "lmrs_batch_mask_info",
    "lmrs_batch_set_history", "lmrs_batch_history", "lmrs_batch_set_penalties", "lmrs_batch_clear_penalties", "lmrs_batch_penalty_info",
    "lmrs_batch_generate",
    "lmrs_batch_set_filters", "lmrs_batch_clear_filters", "lmrs_batch_filter_info", "lmrs_op_filter_rows",
    "lmrs_batch_generate_topp", "lmrs_sampler_candidates", "lmrs_sampler_set_candidates", "lmrs_op_topp_rows", "lmrs_bench_topp_rows",
    "lmrs_automaton_check", "lmrs_automaton_walk", "lmrs_batch_automaton_create", "lmrs_batch_automaton_destroy", "lmrs_batch_attach_automaton",
    "lmrs_batch_automaton_state", "lmrs_batch_automaton_advance", "lmrs_op_automaton_masks",
    "lmrs_last_error",
    "lmrs_op_matmul_q8", "lmrs_op_matmul_q4", "lmrs_op_quantize", "lmrs_op_quantize_q4", "lmrs_op_rmsnorm",
    "lmrs_op_softmax", "lmrs_op_expf", "lmrs_op_tanh_cast", "lmrs_forward_sample", "lmrs_sampler_info", "lmrs_op_sample_mult", "lmrs_op_classifier_argmax", "lmrs_bench_gemv", "lmrs_bench_step", "lmrs_step_info", "lmrs_debug_timeline", "lmrs_debug_kv", "lmrs_debug_inject", "lmrs_last_fill_ms", "lmrs_debug_gemm_tile", "lmrs_debug_w13_quant",
    "lmrs_group_create", "lmrs_group_forward", "lmrs_shard_plan", "lmrs_shard_uses_graph", "lmrs_comm_ranks", "lmrs_p2p_handle", "lmrs_p2p_connect",
    "lmrs_vision_create", "lmrs_vision_destroy", "lmrs_vision_forward",
    "lmrs_processor_create", "lmrs_processor_destroy", "lmrs_processor_forward", "lmrs_processor_hd_transform", "lmrs_rope_terms",
    "lmrs_tokenizer_create", "lmrs_tokenizer_destroy", "lmrs_tokenizer_info", "lmrs_tokenizer_encode", "lmrs_tokenizer_decode",
    "lmrs_sampler_create", "lmrs_sampler_destroy", "lmrs_sampler_sample", "lmrs_sampler_sample_exps", "lmrs_sampler_topp_pairs",
    "lmrs_sampler_exps_prepare", "lmrs_sampler_exps_finish",
]


class TransformerArgs(C.Structure):
    """lmrs_args / TransformerArgs (src/transformer.rs:57-74)."""
    _fields_ = [(n, C.c_uint32) for n in ("dim", "hidden_dim", "n_layers", "n_heads", "head_size", "n_kv_heads", "vocab_size", "seq_len")] + [
        ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float), ("q_type", C.c_uint8), ("model_type", C.c_uint8),
        ("multimodal", C.c_uint8), ("_pad", C.c_uint8), ("group_size", C.c_uint32)]


def build(force: bool = False) -> str:
    """Compile liblmrs_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h", ".inc"))]
    srcs.append(os.path.join(_HERE, "..", "include", "lmrs_hip.h")); srcs.append(os.path.join(CSRC, "Makefile"))     # (the flags are part of the build)
    def stale():
        return not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale():
        # one builder at a time: the ranks of a multi-GPU launch all come through here (bench.py), and two `make`s writing the same
        # objects corrupt them; whoever waited finds the library fresh and skips the build
        import fcntl
        with open(os.path.join(CSRC, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            try:
                if force or stale():
                    subprocess.run(["make", "-s", "-j4", "-C", CSRC], check=True)
            finally:
                fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("LMRS_LIB", LIB_PATH)          # (A/B builds of the same sources: tools/ab_bench.sh)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP extension is mandatory; there is no CPU fallback)")
        L = C.CDLL(path)
        vp, u32, sz, f32p = C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_float)
        L.lmrs_last_error.restype = C.c_char_p
        L.lmrs_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
        L.lmrs_create_sharded.argtypes = [vp, sz, C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp), C.POINTER(sz)]
        L.lmrs_comm_unique_id.argtypes = [vp]
        L.lmrs_destroy.argtypes = [vp]; L.lmrs_destroy.restype = None
        L.lmrs_get_args.argtypes = [vp]; L.lmrs_get_args.restype = C.POINTER(TransformerArgs)
        L.lmrs_forward.argtypes = [vp, u32, u32, C.POINTER(f32p)]
        L.lmrs_forward_argmax.argtypes = [vp, u32, u32, C.POINTER(u32)]
        L.lmrs_get_embeddings.argtypes = [vp, vp, sz, vp]
        L.lmrs_fill_kv_cache.argtypes = [vp, vp, u32, u32, C.POINTER(u32)]
        L.lmrs_generate_greedy.argtypes = [vp, vp, sz, u32, u32, vp, C.POINTER(C.c_double)]
        L.lmrs_forward_tokens.argtypes = [vp, vp, sz, u32, vp]
        L.lmrs_score_tokens.argtypes = [vp, vp, sz, u32, vp, vp, C.POINTER(C.c_double)]
        L.lmrs_score_tokens_topk.argtypes = [vp, vp, sz, u32, u32, vp, vp, C.POINTER(C.c_double), vp, vp, vp]
        L.lmrs_forward_topk.argtypes = [vp, u32, u32, u32, vp, vp]
        L.lmrs_op_topk.argtypes = [C.c_int, vp, sz, sz, u32, vp, vp]
        L.lmrs_prefill_tokens.argtypes = [vp, vp, sz, u32, C.POINTER(u32)]
        L.lmrs_tokens_path.argtypes = [vp, sz, C.POINTER(C.c_int)]
        L.lmrs_verify_tokens.argtypes = [vp, vp, sz, u32, vp, C.POINTER(u32)]
        L.lmrs_draft_lookup.argtypes = [vp, sz, u32, u32, vp, C.POINTER(u32)]
        L.lmrs_generate_speculative.argtypes = [vp, vp, sz, u32, u32, u32, u32, vp, vp, C.POINTER(C.c_double)]
        L.lmrs_debug_gemm_skinny.argtypes = [C.c_int, vp, vp, vp, vp, vp, sz, sz, sz, C.c_int]
        L.lmrs_debug_gemm_wide.argtypes = [C.c_int, vp, vp, vp, vp, vp, sz, sz, sz, C.c_int]
        L.lmrs_batch_create.argtypes = [vp, u32, C.POINTER(vp)]
        L.lmrs_batch_create_wide.argtypes = [vp, u32, C.POINTER(vp)]
        L.lmrs_batch_width.argtypes = [vp, C.POINTER(u32)]
        L.lmrs_batch_create_paged.argtypes = [vp, u32, u32, u32, C.POINTER(vp)]
        L.lmrs_batch_pages.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.lmrs_batch_slot_pages.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32)]
        L.lmrs_batch_release.argtypes = [vp, u32, u32]
        L.lmrs_batch_prefill_form.argtypes = [vp, sz, u32, C.POINTER(u32), C.POINTER(u32)]
        L.lmrs_batch_debug_prefill_table.argtypes = [vp, C.c_int]
        L.lmrs_batch_set_masks.argtypes = [vp, u32, vp, vp]
        L.lmrs_batch_clear_masks.argtypes = [vp, u32, vp]
        L.lmrs_batch_mask_info.argtypes = [vp, u32, C.POINTER(u32)]
        L.lmrs_automaton_check.argtypes = [u32, u32, u32, vp, vp, vp, vp]
        L.lmrs_automaton_walk.argtypes = [u32, u32, u32, vp, vp, vp, u32, vp, sz, C.POINTER(u32), C.POINTER(sz)]
        L.lmrs_batch_automaton_create.argtypes = [vp, u32, u32, vp, vp, vp, C.POINTER(vp)]
        L.lmrs_batch_automaton_destroy.argtypes = [vp, vp]
        L.lmrs_batch_attach_automaton.argtypes = [vp, u32, vp, vp, vp]
        L.lmrs_batch_automaton_state.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_int)]
        L.lmrs_batch_automaton_advance.argtypes = [vp, u32, vp, sz]
        L.lmrs_op_automaton_masks.argtypes = [C.c_int, u32, u32, u32, vp, vp, vp]
        L.lmrs_batch_set_history.argtypes = [vp, u32, u32, vp, sz]
        L.lmrs_batch_history.argtypes = [vp, u32, u32, sz, vp]
        L.lmrs_batch_set_penalties.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.lmrs_batch_clear_penalties.argtypes = [vp, u32, vp]
        L.lmrs_batch_penalty_info.argtypes = [vp, u32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(u32), C.POINTER(C.c_int)]
        L.lmrs_batch_set_filters.argtypes = [vp, u32, vp, vp, vp]
        L.lmrs_batch_clear_filters.argtypes = [vp, u32, vp]
        L.lmrs_batch_filter_info.argtypes = [vp, u32, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.lmrs_op_filter_rows.argtypes = [C.c_int, vp, sz, sz, sz, vp, vp]
        L.lmrs_batch_destroy.argtypes = [vp]; L.lmrs_batch_destroy.restype = None
        L.lmrs_batch_prefill.argtypes = [vp, u32, vp, sz, u32]
        L.lmrs_batch_fork.argtypes = [vp, u32, u32, u32]
        L.lmrs_batch_forward.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.lmrs_batch_generate_greedy.argtypes = [vp, u32, vp, vp, vp, u32, vp, C.POINTER(C.c_double)]
        L.lmrs_batch_generate.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]
        L.lmrs_batch_debug_kv.argtypes = [vp, u32, C.c_int, u32, u32, vp]
        L.lmrs_batch_forward_runs.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
        L.lmrs_batch_forward_sample.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        L.lmrs_batch_forward_runs_sample.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        L.lmrs_batch_prefill_embeddings.argtypes = [vp, u32, vp, u32, u32, vp]
        L.lmrs_batch_forward_runs_embed.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp]
        L.lmrs_batch_forward_runs_embed_sample.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.lmrs_op_sort_candidates.argtypes = [C.c_int, vp, sz, sz, vp, vp]
        L.lmrs_batch_generate_topp.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]
        L.lmrs_sampler_candidates.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.lmrs_sampler_set_candidates.argtypes = [vp, vp]
        L.lmrs_op_topp_rows.argtypes = [C.c_int, sz, sz, vp, vp, vp, vp, vp, vp, vp]
        L.lmrs_bench_topp_rows.argtypes = [C.c_int, sz, sz, sz, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.lmrs_op_sample_rows.argtypes = [C.c_int, vp, sz, sz, vp, vp, vp, vp, vp, vp]
        L.lmrs_sampler_topp_sorted_pairs.argtypes = [vp, vp, sz, C.POINTER(u32)]
        L.lmrs_bench_sample_rows.argtypes = [C.c_int, sz, sz, C.c_int, vp, C.POINTER(C.c_double)]
        L.lmrs_op_matmul_q8.argtypes = [C.c_int, vp, vp, vp, vp, vp, sz, sz, sz, sz]
        L.lmrs_op_matmul_q4.argtypes = [C.c_int, vp, vp, vp, vp, vp, sz, sz, sz]
        L.lmrs_op_quantize.argtypes = [C.c_int, vp, vp, vp, sz, sz]
        L.lmrs_op_quantize_q4.argtypes = [C.c_int, vp, vp, vp, sz, sz]
        L.lmrs_op_rmsnorm.argtypes = [C.c_int, vp, vp, vp, sz, C.c_float, C.c_int]
        L.lmrs_op_softmax.argtypes = [C.c_int, vp, sz]
        L.lmrs_op_expf.argtypes = [C.c_int, vp, vp, sz]
        L.lmrs_op_tanh_cast.argtypes = [C.c_int, vp, vp, sz, C.c_double]
        L.lmrs_bench_gemv.argtypes = [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        L.lmrs_step_info.argtypes = [vp, u32, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        L.lmrs_debug_timeline.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
        L.lmrs_shard_plan.argtypes = [C.POINTER(TransformerArgs), C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.lmrs_shard_uses_graph.argtypes = [vp]
        L.lmrs_comm_ranks.argtypes = [vp]
        L.lmrs_group_create.argtypes = [vp, sz, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(sz)]
        L.lmrs_group_forward.argtypes = [C.POINTER(vp), C.c_int, u32, u32, C.POINTER(f32p), C.POINTER(u32)]
        L.lmrs_vision_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
        L.lmrs_vision_destroy.argtypes = [vp]
        L.lmrs_vision_destroy.restype = None
        L.lmrs_vision_forward.argtypes = [vp, vp, u32, vp, C.POINTER(u32)]
        L.lmrs_processor_create.argtypes = [vp, sz, C.c_int, C.POINTER(vp), C.POINTER(sz)]
        L.lmrs_processor_destroy.argtypes = [vp]
        L.lmrs_processor_destroy.restype = None
        L.lmrs_processor_forward.argtypes = [vp, vp, u32, u32, u32, u32, u32, vp, C.POINTER(u32)]
        L.lmrs_processor_hd_transform.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, C.POINTER(u32)]
        L.lmrs_rope_terms.argtypes = [C.POINTER(TransformerArgs), u32, u32, f32p, f32p]
        L.lmrs_tokenizer_create.argtypes = [vp, sz, C.POINTER(vp)]
        L.lmrs_tokenizer_destroy.argtypes = [vp]; L.lmrs_tokenizer_destroy.restype = None
        L.lmrs_tokenizer_info.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
        L.lmrs_tokenizer_encode.argtypes = [vp, C.c_char_p, sz, C.c_int, C.c_int, C.c_int, C.c_int, vp, sz, C.POINTER(sz)]
        L.lmrs_tokenizer_decode.argtypes = [vp, u32, C.c_char_p, sz, C.POINTER(sz)]
        L.lmrs_sampler_create.argtypes = [u32, C.c_float, C.c_float, C.c_uint64, C.POINTER(vp)]
        L.lmrs_sampler_destroy.argtypes = [vp]; L.lmrs_sampler_destroy.restype = None
        L.lmrs_sampler_sample.argtypes = [vp, vp, C.POINTER(u32)]
        L.lmrs_sampler_topp_pairs.argtypes = [vp, vp, sz, C.POINTER(u32)]
        L.lmrs_sampler_sample_exps.argtypes = [vp, vp, C.POINTER(u32)]
        L.lmrs_sampler_exps_prepare.argtypes = [vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_size_t)]
        L.lmrs_sampler_exps_finish.argtypes = [vp, vp, vp, C.POINTER(u32)]
        L.lmrs_sampler_info.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.lmrs_forward_sample.argtypes = [vp, u32, u32, vp, C.POINTER(u32)]
        L.lmrs_op_sample_mult.argtypes = [C.c_int, vp, sz, C.c_float, C.c_float, C.POINTER(u32)]
        L.lmrs_debug_kv.argtypes = [vp, C.c_int, u32, u32, vp]
        L.lmrs_debug_inject.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.lmrs_last_fill_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.lmrs_debug_gemm_tile.argtypes = [u32, u32, u32, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.lmrs_debug_w13_quant.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp, sz, sz, sz, C.c_int]
        L.lmrs_p2p_handle.argtypes = [vp, vp]
        L.lmrs_p2p_connect.argtypes = [vp, vp]
        L.lmrs_bench_step.argtypes = [vp, u32, C.c_int, vp, vp, vp]
        L.lmrs_op_classifier_argmax.argtypes = [C.c_int, vp, vp, vp, vp, sz, sz, C.c_float, C.POINTER(u32), vp]
        _lib = L
    return _lib


class LmrsError(RuntimeError):
    """The reference panics (assert!/expect); the C ABI returns a status and we raise."""


def _chk(rc):
    if rc:
        raise LmrsError(lib().lmrs_last_error().decode())


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


class Transformer:
    """Drop-in for lmrs::transformer::Transformer on one MI355X.

    Transformer(data) -> like Transformer::new(&mmap): `data` is the LMRS image (bytes-like /
    numpy uint8 / np.memmap).  `.bytes_consumed` is the second element of the reference's tuple.
    """

    def __init__(self, data, device: int = 0, rank: int = 0, world: int = 1, unique_id: bytes | None = None):
        image = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8)
        h, used = C.c_void_p(), C.c_size_t()
        if world == 1 and unique_id is None:
            _chk(lib().lmrs_create(_p(image), image.size, device, C.byref(h), C.byref(used)))
        else:
            uid = C.create_string_buffer(unique_id, 128) if unique_id else None
            _chk(lib().lmrs_create_sharded(_p(image), image.size, device, rank, world, uid, C.byref(h), C.byref(used)))
        self._h = h
        self.bytes_consumed = used.value
        self.args = lib().lmrs_get_args(h).contents

    def close(self):
        if getattr(self, "_h", None):
            lib().lmrs_destroy(self._h)
            self._h = None

    __del__ = close

    def forward(self, token: int, pos: int) -> np.ndarray:
        """-> logits view (vocab_size f32, pinned host memory owned by the model, valid until the next call)."""
        p = C.POINTER(C.c_float)()
        _chk(lib().lmrs_forward(self._h, token, pos, C.byref(p)))
        return np.ctypeslib.as_array(p, shape=(self.args.vocab_size,))

    def forward_argmax(self, token: int, pos: int) -> int:
        n = C.c_uint32()
        _chk(lib().lmrs_forward_argmax(self._h, token, pos, C.byref(n)))
        return n.value

    def forward_sample(self, token: int, pos: int, sampler: "Sampler") -> int:
        """forward + Sampler::sample: temperature 0 -> the fused argmax; else scaling / max / exp on the device, the sequential chains on the host, the sort of
        many top-p candidates on the device again (lmrs_forward_sample)"""
        n = C.c_uint32()
        _chk(lib().lmrs_forward_sample(self._h, token, pos, sampler._h, C.byref(n)))
        return n.value

    def get_embeddings(self, tokens) -> np.ndarray:
        t = np.ascontiguousarray(tokens, np.uint32)
        out = np.empty(t.size * self.args.dim, np.float32)
        _chk(lib().lmrs_get_embeddings(self._h, _p(t), t.size, _p(out)))
        return out

    def fill_kv_cache(self, embeddings: np.ndarray, curr_pos: int) -> int:
        if embeddings.dtype != np.float32 or not embeddings.flags.c_contiguous or embeddings.size % self.args.dim:
            raise LmrsError("embeddings must be a contiguous float32 array of n*dim elements")
        newp = C.c_uint32()
        _chk(lib().lmrs_fill_kv_cache(self._h, _p(embeddings), embeddings.size // self.args.dim, curr_pos, C.byref(newp)))
        return newp.value

    def generate_greedy(self, prompt, n_new: int, start_pos: int = 0, timing: bool = False):
        """chat.rs:188-222 on token IDs: returns the n_new greedy tokens (and device seconds if timing)."""
        pr = np.ascontiguousarray(prompt, np.uint32)
        out = np.zeros(n_new, np.uint32)
        sec = C.c_double()
        _chk(lib().lmrs_generate_greedy(self._h, _p(pr), pr.size, n_new, start_pos, _p(out), C.byref(sec)))
        return (out, sec.value) if timing else out

    def forward_tokens(self, tokens, start_pos: int = 0) -> np.ndarray:
        """-> float32 [n, vocab_size]: row t = forward(tokens[t], start_pos + t) after the calls for 0..t-1 (lmrs_forward_tokens)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        out = np.empty((t.size, self.args.vocab_size), np.float32)
        _chk(lib().lmrs_forward_tokens(self._h, _p(t), t.size, start_pos, _p(out)))
        return out

    def score(self, tokens, start_pos: int = 0):
        """-> (logprobs float32 [n-1]: log softmax(logits_t)[tokens[t+1]], argmax uint32 [n], sum of the log-probabilities in double)
        for the same pass as forward_tokens, the logits kept on the device (lmrs_score_tokens)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        lp = np.empty(max(t.size - 1, 0), np.float32); am = np.empty(t.size, np.uint32); s = C.c_double()
        _chk(lib().lmrs_score_tokens(self._h, _p(t), t.size, start_pos, _p(lp), _p(am), C.byref(s)))
        return lp, am, s.value

    def score_topk(self, tokens, k: int, start_pos: int = 0):
        """score() with the k most likely next tokens of every position -> (logprobs, argmax, sum - bit for bit score()'s -, topk_idx uint32 [n, k],
        topk_logprob float32 [n, k], target_rank uint32 [n-1]).  Order: larger logit first, equal logits by ascending index, NaNs last (a NaN at
        index 0 first, as the argmax has it); topk_logprob shares logprobs' maximum and sum; target_rank[t] counts the candidates that precede
        tokens[t+1], whatever k is (lmrs_score_tokens_topk)."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        lp = np.empty(max(t.size - 1, 0), np.float32); am = np.empty(t.size, np.uint32); s = C.c_double()
        ti = np.empty((t.size, max(int(k), 0)), np.uint32); tl = np.empty(ti.shape, np.float32); rk = np.empty(lp.size, np.uint32)
        _chk(lib().lmrs_score_tokens_topk(self._h, _p(t), t.size, start_pos, k, _p(lp), _p(am), C.byref(s), _p(ti), _p(tl), _p(rk)))
        return lp, am, s.value, ti, tl, rk

    def forward_topk(self, token: int, pos: int, k: int):
        """forward() with the selection on the device -> (idx uint32 [k], raw logits float32 [k]) in score_topk's order; 2k words cross to the
        host, the state afterwards is forward()'s (lmrs_forward_topk)."""
        idx = np.empty(max(int(k), 0), np.uint32); val = np.empty(idx.size, np.float32)
        _chk(lib().lmrs_forward_topk(self._h, token, pos, k, _p(idx), _p(val)))
        return idx, val

    def prefill_tokens(self, tokens, start_pos: int = 0) -> int:
        """forward(tokens[t], start_pos + t) for every t with the logits discarded: the K/V rows of a prompt, the token ids going to the
        device and the layers over the whole run where tokens_path says so (lmrs_prefill_tokens) -> start_pos + n"""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        newp = C.c_uint32()
        _chk(lib().lmrs_prefill_tokens(self._h, _p(t), t.size, start_pos, C.byref(newp)))
        return newp.value

    def tokens_path(self, n: int) -> bool:
        """True: prefill_tokens (and generate_greedy's prompt of n + 1 tokens) runs a run of n tokens as one batched pass (lmrs_tokens_path)"""
        b = C.c_int()
        _chk(lib().lmrs_tokens_path(self._h, n, C.byref(b)))
        return bool(b.value)

    def verify_tokens(self, tokens, start_pos: int = 0):
        """tokens[0] = the last confirmed token at start_pos, tokens[1:] = drafts (2 <= n <= 16) -> (argmax uint32 [n]: forward_argmax of every
        position, n_accept: the leading drafts with tokens[t+1] == argmax[t]) in one pass over the weights where score() would run batched
        (lmrs_verify_tokens).  The next pass starts at start_pos + n_accept + 1 with argmax[n_accept]."""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        am = np.empty(t.size, np.uint32); acc = C.c_uint32()
        _chk(lib().lmrs_verify_tokens(self._h, _p(t), t.size, start_pos, _p(am), C.byref(acc)))
        return am, acc.value

    def generate_speculative(self, prompt, n_new: int, start_pos: int = 0, max_draft: int = 7, ngram_max: int = 3, timing: bool = False):
        """generate_greedy's tokens, bit for bit, by prompt-lookup drafting (draft_lookup) and verify passes (lmrs_generate_speculative) ->
        (tokens uint32 [n_new], stats uint32 [4]: verify passes, drafted, accepted, plain decode steps; passes + accepted + plain == n_new)
        (and host seconds if timing)."""
        pr = np.ascontiguousarray(prompt, np.uint32).reshape(-1)
        out = np.zeros(n_new, np.uint32); st = np.zeros(4, np.uint32); sec = C.c_double()
        _chk(lib().lmrs_generate_speculative(self._h, _p(pr), pr.size, n_new, start_pos, max_draft, ngram_max, _p(out), _p(st), C.byref(sec)))
        return (out, st, sec.value) if timing else (out, st)

    def kv_row(self, which: int, layer: int, pos: int) -> np.ndarray:
        """Verification aid: one KV-cache row in the reference's layout (which: 0 key, 1 value)."""
        out = np.empty(self.args.n_kv_heads * self.args.head_size, np.float32)
        _chk(lib().lmrs_debug_kv(self._h, which, layer, pos, _p(out)))
        return out

    def last_fill_ms(self) -> float:
        """device milliseconds of the last batched fill_kv_cache without its host <-> device copies (lmrs_last_fill_ms)"""
        ms = C.c_double()
        _chk(lib().lmrs_last_fill_ms(self._h, C.byref(ms)))
        return ms.value

    def debug_inject(self, what: int, a: int = 0, b: int = 0) -> None:
        """Fault injection for the multi-GPU tests (include/lmrs_hip.h: lmrs_debug_inject)."""
        _chk(lib().lmrs_debug_inject(self._h, what, a, b))

    def p2p_handle(self) -> bytes:
        """Peer-to-peer sharded context: the 64-byte IPC handle of this rank's exchange arena (send it to every peer)."""
        buf = C.create_string_buffer(64)
        _chk(lib().lmrs_p2p_handle(self._h, buf))
        return buf.raw

    def p2p_connect(self, handles) -> None:
        """handles: the `world` handles in rank order."""
        blob = b"".join(handles)
        _chk(lib().lmrs_p2p_connect(self._h, C.create_string_buffer(blob, len(blob))))

    def comm_ranks(self) -> int:
        """ranks of the RCCL communicator (ncclCommCount); 0: none (one GPU / peer-to-peer transport)"""
        return lib().lmrs_comm_ranks(self._h)

    def shard_uses_graph(self) -> int:
        return lib().lmrs_shard_uses_graph(self._h)

    # ---- measurement hooks
    def bench_gemv(self, iters: int = 5):
        """-> {shape: (sum_us, sum_bytes, launches)} over `iters` GEMV-only passes of one decode step."""
        us, b, n = (C.c_double * 5)(), (C.c_double * 5)(), (C.c_int * 5)()
        _chk(lib().lmrs_bench_gemv(self._h, iters, us, b, n))
        names = ["qkv", "wo", "w1w3", "w2", "classifier"]
        return {names[k]: (us[k], b[k], n[k]) for k in range(5)}

    def bench_step(self, pos: int, iters: int = 8):
        """Per-kernel durations of the real decode step (eager replay with events on every dispatch) -> {kind: (us, bytes, launches)}."""
        us = np.zeros(9, np.float64); b = np.zeros(9, np.float64); n = np.zeros(9, np.int32)
        _chk(lib().lmrs_bench_step(self._h, pos, iters, _p(us), _p(b), _p(n)))
        names = ("qkv", "attention", "wo", "w1w3", "w2", "classifier", "argmax", "glue", "exchange")
        return {k: (float(us[i]), float(b[i]), int(n[i])) for i, k in enumerate(names) if n[i]}

    def debug_timeline(self):
        """-> uint64[n_kernels, 8] wall-clock stamps (10 ns units) of the last decode step (needs LMRS_DEBUG_TIMELINE=1)."""
        buf = np.zeros((1024, 8), np.uint64); n = C.c_int()
        _chk(lib().lmrs_debug_timeline(self._h, _p(buf), 1024, C.byref(n)))
        return buf[: n.value]

    def step_info(self, pos: int):
        n, b = C.c_int(), C.c_double()
        _chk(lib().lmrs_step_info(self._h, pos, C.byref(n), C.byref(b)))
        return n.value, b.value


def _is_embed_run(rows) -> bool:
    """a run's rows are embeddings: a 2-D float32 array (token ids come as lists or integer arrays)"""
    return isinstance(rows, np.ndarray) and rows.ndim == 2 and rows.dtype == np.float32


def pack_mask(allowed) -> np.ndarray:
    """bool [..., vocab_size] (true = the token is allowed) -> uint32 [..., W], W = (vocab_size + 31) // 32: bit (t & 31) of word (t >> 5) is token t,
    the bits at and above vocab_size zero (the layout lmrs_batch_set_masks takes)"""
    a = np.asarray(allowed)
    if a.dtype != np.bool_ or a.ndim < 1:
        raise LmrsError("pack_mask takes a bool array whose last axis is the vocabulary")
    V = a.shape[-1]
    W = (V + 31) // 32
    padded = np.zeros(a.shape[:-1] + (W * 32,), np.uint8)
    padded[..., :V] = a
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view("<u4").astype(np.uint32, copy=False)


def unpack_mask(words, vocab_size: int) -> np.ndarray:
    """pack_mask's inverse: uint32 [..., W] -> bool [..., vocab_size]"""
    w = np.ascontiguousarray(words, np.uint32)
    if w.ndim < 1 or w.shape[-1] != (vocab_size + 31) // 32:
        raise LmrsError(f"a mask of vocab_size = {vocab_size} holds {(vocab_size + 31) // 32} words")
    return np.unpackbits(w.astype("<u4", copy=False).view(np.uint8), axis=-1, bitorder="little")[..., :vocab_size].astype(np.bool_)


BATCH_CTX = 0xFFFFFFFF        # Batch.fork's src: the model's own cache (LMRS_BATCH_CTX)
TOKEN_NONE = 0xFFFFFFFF       # Batch.history / set_history: a position whose token is unknown, or an embedding row (LMRS_TOKEN_NONE)
STOP_MAX = 16                 # Batch.generate: the most stop tokens a row takes (LMRS_STOP_MAX)
FINISH_BUDGET, FINISH_STOP = 0, 1     # Batch.generate's finish codes (LMRS_FINISH_BUDGET / LMRS_FINISH_STOP)
FINISH_NO_CANDIDATE = 2               # Batch.generate_topp: a top-p row's step found no candidate above the cutoff (LMRS_FINISH_NO_CANDIDATE)
FINISH_FINAL = 3                      # Batch.generate / generate_topp: the row's automaton reached a final state (LMRS_FINISH_FINAL)
STATE_DEAD = 0xFFFFFFFF               # TokenAutomaton.next: no transition - the class's tokens are not allowed in that state (LMRS_STATE_DEAD)
AUTOMATA_MAX = 16                     # the automata a batch holds at a time (LMRS_AUTOMATA_MAX)


class TokenAutomaton:
    """A DFA over tokens in compressed form (include/lmrs_hip.h): class_of uint16 [vocab_size], next uint32 [n_states, n_classes] - a state or
    STATE_DEAD - and final bool [n_states].  Token t is allowed in state q iff next[q, class_of[t]] != STATE_DEAD, and choosing it moves there.
    Every state that is not final must allow a token; a final state may allow none.  Host arithmetic only: no GPU is touched here."""

    def __init__(self, class_of, next, final=None):
        self.class_of = np.ascontiguousarray(class_of, np.uint16).reshape(-1)
        nx = np.ascontiguousarray(next, np.uint32)
        if nx.ndim != 2:
            raise LmrsError("next must be [n_states, n_classes]")
        self.next = nx
        self.final = np.zeros(nx.shape[0], np.uint8) if final is None else np.ascontiguousarray(np.asarray(final).astype(bool), np.uint8).reshape(-1)
        if self.final.size != nx.shape[0]:
            raise LmrsError("final must hold one flag per state")

    vocab_size = property(lambda self: int(self.class_of.size))
    n_states = property(lambda self: int(self.next.shape[0]))
    n_classes = property(lambda self: int(self.next.shape[1]))

    def check(self) -> np.ndarray:
        """The tables' rules -> the allowed tokens of every state, uint32 [n_states]; a broken rule raises with the state, class or token named
        (lmrs_automaton_check)"""
        n = np.zeros(self.n_states, np.uint32)
        _chk(lib().lmrs_automaton_check(self.vocab_size, self.n_states, self.n_classes, _p(self.class_of), _p(self.next), _p(self.final), _p(n)))
        return n

    def walk(self, state: int, tokens):
        """tokens from `state` -> (state behind them, tokens walked, ok): ok false - the walk stopped in front of a token its state does not allow,
        and the state is the one in front of that token (lmrs_automaton_walk)"""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        q, k = C.c_uint32(), C.c_size_t()
        rc = lib().lmrs_automaton_walk(self.vocab_size, self.n_states, self.n_classes, _p(self.class_of), _p(self.next), _p(self.final), state,
                                       _p(t) if t.size else None, t.size, C.byref(q), C.byref(k))
        if rc and not (k.value < t.size and " is not allowed in state " in lib().lmrs_last_error().decode()):
            _chk(rc)                                             # (an argument out of range, not a disallowed token)
        return q.value, k.value, rc == 0

    def allowed(self, state: int) -> np.ndarray:
        """bool [vocab_size]: the tokens `state` allows"""
        return self.next[state][self.class_of] != STATE_DEAD

    @classmethod
    def from_transitions(cls, vocab_size: int, table, final=None) -> "TokenAutomaton":
        """table: dense uint32 [n_states, vocab_size] (a state or STATE_DEAD per token), or a list of dicts {token: state}, one per state.  Tokens whose
        columns are identical share a class (at most 65536 classes)"""
        if isinstance(table, np.ndarray):
            dense = np.ascontiguousarray(table, np.uint32)
        else:
            dense = np.full((len(table), vocab_size), STATE_DEAD, np.uint32)
            for q, row in enumerate(table):
                for t, to in row.items():
                    dense[q, t] = to
        if dense.ndim != 2 or dense.shape[1] != vocab_size:
            raise LmrsError(f"a dense table must be [n_states, vocab_size = {vocab_size}]")
        cols, inverse = np.unique(dense.T, axis=0, return_inverse=True)
        if cols.shape[0] > 65536:
            raise LmrsError(f"{cols.shape[0]} distinct token columns: more than 65536 classes")
        return cls(inverse.reshape(-1).astype(np.uint16), np.ascontiguousarray(cols.T), final)

    @classmethod
    def from_sequences(cls, vocab_size: int, seqs) -> "TokenAutomaton":
        """"Choose one of these multi-token labels": a trie over the token sequences, state 0 its root, every leaf final.  No sequence may be empty
        or a proper prefix of another (its end would be an inner state)"""
        rows, final = [{}], [False]
        for seq in seqs:
            seq = [int(t) for t in seq]
            if not seq:
                raise LmrsError("from_sequences: an empty sequence")
            q = 0
            for t in seq:
                if not 0 <= t < vocab_size:
                    raise LmrsError(f"from_sequences: token {t} is not below vocab_size = {vocab_size}")
                if final[q]:
                    raise LmrsError("from_sequences: a sequence is a proper prefix of another")
                if t not in rows[q]:
                    rows[q][t] = len(rows); rows.append({}); final.append(False)
                q = rows[q][t]
            if rows[q]:
                raise LmrsError("from_sequences: a sequence is a proper prefix of another")
            final[q] = True
        return cls.from_transitions(vocab_size, rows, final)


class Batch:
    """n_slots (1 .. 16) more K/V caches beside a Transformer's own, stepped together: one pass over the weights serves one token of up to 16
    DIFFERENT sequences, each at its own position (lmrs_batch_*).  Every result is bit for bit what forward / forward_argmax give on a model that
    holds only that sequence.  The model's own cache is untouched by every call here; close the batch before the model.
    wide=True: up to 64 slots, and forward / generate_greedy / forward_runs / forward_runs_sample take up to 64 rows or runs a call
    (lmrs_batch_create_wide; forward_sample keeps 16 rows).
    page_len= and n_pages= (both or neither; wide= is then ignored): a PAGED batch, wide, whose slots draw pages of page_len positions (64, 128, 256,
    512 or 1024) from one pool of n_pages pages instead of holding a whole cache each: fork shares whole pages, a write un-shares the page it
    touches, release gives pages back.  Without release every result is bit for bit a wide batch's (lmrs_batch_create_paged)."""

    def __init__(self, model: Transformer, n_slots: int, wide: bool = False, *, page_len=None, n_pages=None):
        h = C.c_void_p()
        if (page_len is None) != (n_pages is None):
            raise LmrsError("page_len and n_pages must be given together")
        if page_len is not None:
            _chk(lib().lmrs_batch_create_paged(model._h, n_slots, page_len, n_pages, C.byref(h)))
        else:
            _chk((lib().lmrs_batch_create_wide if wide else lib().lmrs_batch_create)(model._h, n_slots, C.byref(h)))
        self._h, self.model, self.n_slots = h, model, n_slots

    def pages(self):
        """A paged batch's pool -> (page_len, n_pages, n_free) (lmrs_batch_pages)"""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(lib().lmrs_batch_pages(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def slot_pages(self, slot: int):
        """The pages `slot` holds and how many of them have more than one holder -> (held, shared) (lmrs_batch_slot_pages)"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(lib().lmrs_batch_slot_pages(self._h, slot, C.byref(a), C.byref(b)))
        return a.value, b.value

    def release(self, slot: int, n_pos: int = 0) -> None:
        """Keep positions [0, n_pos) of `slot` (0 empties it): the pages behind them go back to the pool once nobody holds them (lmrs_batch_release)"""
        _chk(lib().lmrs_batch_release(self._h, slot, n_pos))

    def prefill_form(self, n: int, start_pos: int = 0):
        """How prefill / prefill_embeddings would run n rows at start_pos on this batch -> (n_chunks, n_block): passes of at most 512 rows, and how many
        of them take block attention (64-query blocks); the others take one workgroup per (head, row).  Host arithmetic only (lmrs_batch_prefill_form)"""
        a, b = C.c_uint32(), C.c_uint32()
        _chk(lib().lmrs_batch_prefill_form(self._h, n, start_pos, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_prefill_table(self, force: bool = True) -> None:
        """Test / A-B aid: every prompt chunk of this PAGED batch takes the table pass from now on (force false: the library's rule again).  Refused
        on a batch that is not paged (lmrs_batch_debug_prefill_table)"""
        _chk(lib().lmrs_batch_debug_prefill_table(self._h, 1 if force else 0))

    def set_masks(self, slots, masks) -> None:
        """Allowed-token masks for `slots`, one row of `masks` each: bool [n, vocab_size] (true = allowed) or packed uint32 [n, W] (pack_mask).  While a
        slot has a mask, every output of its rows in any call here - logits, argmax, top-k, sampled token - comes from the row's logits with the
        disallowed entries -inf; the mask stays until it is replaced or cleared (lmrs_batch_set_masks)"""
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)
        V = self.model.args.vocab_size
        m = np.asarray(masks)
        if m.dtype == np.bool_:
            if m.ndim != 2 or m.shape != (s.size, V):
                raise LmrsError(f"bool masks must be [{s.size}, vocab_size = {V}]")
            m = pack_mask(m)
        m = np.ascontiguousarray(m, np.uint32)
        if m.ndim != 2 or m.shape != (s.size, (V + 31) // 32):
            raise LmrsError(f"packed masks must be [{s.size}, {(V + 31) // 32}] uint32 words")
        _chk(lib().lmrs_batch_set_masks(self._h, s.size, _p(s) if s.size else None, _p(m) if s.size else None))

    def clear_masks(self, slots=None) -> None:
        """The named slots lose their masks; None: every slot (lmrs_batch_clear_masks)"""
        if slots is None:
            _chk(lib().lmrs_batch_clear_masks(self._h, 0, None))
            return
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)
        if s.size:                                              # (an empty list names no slot; n == 0 in the C call means all of them)
            _chk(lib().lmrs_batch_clear_masks(self._h, s.size, _p(s)))

    def mask_info(self, slot: int):
        """The number of tokens `slot`'s mask allows, or None when the slot has no mask (lmrs_batch_mask_info)"""
        n = C.c_uint32()
        _chk(lib().lmrs_batch_mask_info(self._h, slot, C.byref(n)))
        return n.value or None

    def automaton(self, ta: TokenAutomaton):
        """`ta` on the device for this batch -> a handle for attach: its tables uploaded, the per-state masks built there; at most AUTOMATA_MAX at a
        time (lmrs_batch_automaton_create).  drop_automaton frees one that no slot is attached to; closing the batch frees all"""
        if ta.vocab_size != self.model.args.vocab_size:
            raise LmrsError(f"the automaton is over {ta.vocab_size} tokens, the model's vocab_size is {self.model.args.vocab_size}")
        h = C.c_void_p()
        _chk(lib().lmrs_batch_automaton_create(self._h, ta.n_states, ta.n_classes, _p(ta.class_of), _p(ta.next), _p(ta.final), C.byref(h)))
        return h

    def drop_automaton(self, handle) -> None:
        """lmrs_batch_automaton_destroy: refused while a slot is attached to it"""
        _chk(lib().lmrs_batch_automaton_destroy(self._h, handle))

    def attach(self, slots, automata, states=0) -> None:
        """Slot slots[i] gets automaton automata[i] (a handle of automaton(); None detaches) in start state states[i]; one handle / one state serves
        every slot.  From then on every output of the slot's rows is computed under the mask of its current state; generate / generate_topp move the
        state with every token they choose, advance moves it by hand (lmrs_batch_attach_automaton)"""
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)
        hs = list(automata) if isinstance(automata, (list, tuple)) else [automata] * s.size
        q = np.asarray(states)
        q = np.ascontiguousarray(np.full(s.size, q) if q.ndim == 0 else q.reshape(-1), np.uint32)
        if len(hs) != s.size or q.size != s.size:
            raise LmrsError("attach takes one automaton and one state per slot")
        arr = (C.c_void_p * max(s.size, 1))(*[None if h is None else h for h in hs])
        _chk(lib().lmrs_batch_attach_automaton(self._h, s.size, _p(s) if s.size else None, C.cast(arr, C.c_void_p), _p(q) if s.size else None))

    def automaton_state(self, slot: int):
        """-> (state, n_allowed, is_final) of `slot`'s automaton, or None when the slot has none (lmrs_batch_automaton_state)"""
        q, n, f = C.c_uint32(), C.c_uint32(), C.c_int()
        _chk(lib().lmrs_batch_automaton_state(self._h, slot, C.byref(q), C.byref(n), C.byref(f)))
        return None if q.value == STATE_DEAD else (q.value, n.value, bool(f.value))

    def advance(self, slot: int, tokens) -> None:
        """The slot's state moves over `tokens`; a token its state does not allow raises and changes nothing (lmrs_batch_automaton_advance)"""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        _chk(lib().lmrs_batch_automaton_advance(self._h, slot, _p(t) if t.size else None, t.size))

    def set_penalties(self, slots, repetition=1.0, presence=0.0, frequency=0.0, out_from=0) -> None:
        """Repetition / presence / frequency penalties for `slots`; a scalar serves every slot, an array gives one value each.  While a slot has
        them, every output of its rows in any call here comes from the row's logits changed by the rule of include/lmrs_hip.h over the tokens the
        slot has seen (history): tokens seen anywhere are divided / multiplied by `repetition`, tokens seen at positions >= out_from lose
        frequency * count + presence.  The first call switches the batch's token record on (lmrs_batch_set_penalties)"""
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)

        def per_slot(name, v, dtype):
            a = np.asarray(v)
            if a.ndim == 0:
                a = np.full(s.size, v)
            a = a.reshape(-1)
            if a.size != s.size:
                raise LmrsError(f"{name} must be a scalar or hold one value per slot ({s.size}), got {a.size}")
            if dtype == np.uint32 and a.size and (np.any(a < 0) or np.any(a != np.floor(a))):
                raise LmrsError(f"{name} must hold whole numbers >= 0")
            return np.ascontiguousarray(a, dtype)
        r, p, f = (per_slot(n, v, np.float32) for n, v in (("repetition", repetition), ("presence", presence), ("frequency", frequency)))
        o = per_slot("out_from", out_from, np.uint32)
        _chk(lib().lmrs_batch_set_penalties(self._h, s.size, *((_p(x) if s.size else None) for x in (s, r, p, f, o))))

    def clear_penalties(self, slots=None) -> None:
        """The named slots lose their penalties; None: every slot.  The token record stays (lmrs_batch_clear_penalties)"""
        if slots is None:
            _chk(lib().lmrs_batch_clear_penalties(self._h, 0, None))
            return
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)
        if s.size:                                              # (an empty list names no slot; n == 0 in the C call means all of them)
            _chk(lib().lmrs_batch_clear_penalties(self._h, s.size, _p(s)))

    def penalty_info(self, slot: int):
        """`slot`'s penalties -> dict(repetition, presence, frequency, out_from, active); active is False while they change no logit
        (lmrs_batch_penalty_info)"""
        r, p, f, o, a = C.c_float(), C.c_float(), C.c_float(), C.c_uint32(), C.c_int()
        _chk(lib().lmrs_batch_penalty_info(self._h, slot, C.byref(r), C.byref(p), C.byref(f), C.byref(o), C.byref(a)))
        return dict(repetition=r.value, presence=p.value, frequency=f.value, out_from=o.value, active=bool(a.value))

    def set_filters(self, slots, top_k=0, min_gap=float("inf")) -> None:
        """Candidate filters for `slots`; a scalar serves every slot, an array gives one value each.  While a slot has them, every output of its rows in
        any call here but generate_greedy comes from the row with every logit outside the first top_k candidates (0: off) and every logit more than
        min_gap below the largest (inf: off; min_p_gap turns a min_p into it) set to -inf, behind the penalties and the mask (include/lmrs_hip.h: the
        rule).  (0, inf) is the same as clearing (lmrs_batch_set_filters)"""
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)

        def per_slot(name, v, dtype):
            a = np.asarray(v)
            if a.ndim == 0:
                a = np.full(s.size, v)
            a = a.reshape(-1)
            if a.size != s.size:
                raise LmrsError(f"{name} must be a scalar or hold one value per slot ({s.size}), got {a.size}")
            if dtype == np.uint32 and a.size and (np.any(a < 0) or np.any(a != np.floor(a)) or np.any(a > 0xFFFFFFFF)):
                raise LmrsError(f"{name} must hold whole numbers >= 0 and below 2^32")
            return np.ascontiguousarray(a, dtype)
        k, g = per_slot("top_k", top_k, np.uint32), per_slot("min_gap", min_gap, np.float32)
        _chk(lib().lmrs_batch_set_filters(self._h, s.size, *((_p(x) if s.size else None) for x in (s, k, g))))

    def clear_filters(self, slots=None) -> None:
        """The named slots lose their filters; None: every slot (lmrs_batch_clear_filters)"""
        if slots is None:
            _chk(lib().lmrs_batch_clear_filters(self._h, 0, None))
            return
        s = np.ascontiguousarray(slots, np.uint32).reshape(-1)
        if s.size:                                              # (an empty list names no slot; n == 0 in the C call means all of them)
            _chk(lib().lmrs_batch_clear_filters(self._h, s.size, _p(s)))

    def filter_info(self, slot: int):
        """`slot`'s filters -> dict(top_k, min_gap, active); active is False while they can clear no logit (lmrs_batch_filter_info)"""
        k, g, a = C.c_uint32(), C.c_float(), C.c_int()
        _chk(lib().lmrs_batch_filter_info(self._h, slot, C.byref(k), C.byref(g), C.byref(a)))
        return dict(top_k=k.value, min_gap=g.value, active=bool(a.value))

    def set_history(self, slot: int, tokens=(), start_pos: int = 0) -> None:
        """The token record of `slot` from start_pos on = tokens (TOKEN_NONE: unknown) - what the caller knows of positions written before the record
        existed.  With no tokens the call only switches the record on (lmrs_batch_set_history)"""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        _chk(lib().lmrs_batch_set_history(self._h, slot, start_pos, _p(t) if t.size else None, t.size))

    def history(self, slot: int, n: int, start_pos: int = 0):
        """The token record of `slot` at positions [start_pos, start_pos + n) -> uint32 [n], TOKEN_NONE where the token is unknown or the row was an
        embedding; an error on a batch that keeps no record (lmrs_batch_history)"""
        if n < 0:
            raise LmrsError("n must not be negative")
        out = np.empty(n, np.uint32)
        _chk(lib().lmrs_batch_history(self._h, slot, start_pos, n, _p(out) if n else None))
        return out

    @property
    def width(self) -> int:
        """The most rows (forward, generate_greedy) and runs (forward_runs) a call takes: 16, or 64 for a wide batch (lmrs_batch_width)"""
        w = C.c_uint32()
        _chk(lib().lmrs_batch_width(self._h, C.byref(w)))
        return w.value

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self.model, "_h", None):
                lib().lmrs_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def prefill(self, slot: int, tokens, start_pos: int = 0) -> int:
        """Transformer.prefill_tokens into `slot`'s cache -> start_pos + n (lmrs_batch_prefill)"""
        t = np.ascontiguousarray(tokens, np.uint32).reshape(-1)
        _chk(lib().lmrs_batch_prefill(self._h, slot, _p(t), t.size, start_pos))
        return start_pos + t.size

    def prefill_embeddings(self, slot: int, embeddings, start_pos: int = 0, residual: bool = False):
        """ONE Transformer.fill_kv_cache call into `slot`'s cache: embeddings float32 [n, dim], taken as given and never written -> start_pos + n, or
        with residual=True the tuple (start_pos + n, float32 [n, dim] as the reference leaves its mutated argument); without it nothing is downloaded
        (lmrs_batch_prefill_embeddings)"""
        e = np.ascontiguousarray(embeddings, np.float32)
        dim = self.model.args.dim
        if e.size % dim:
            raise LmrsError(f"embeddings must hold whole rows of dim = {dim} floats")
        n = e.size // dim
        res = np.empty((n, dim), np.float32) if residual else None
        _chk(lib().lmrs_batch_prefill_embeddings(self._h, slot, _p(e) if n else None, n, start_pos, _p(res) if residual else None))
        return (start_pos + n, res) if residual else start_pos + n

    def _run_rows(self, runs):
        """the rows of runs whose third entry is a token list or a 2-D float32 array of embedding rows -> (run_len, run_kind, tokens, embeddings)"""
        dim = self.model.args.dim
        n, kind, toks, embs = [], [], [], []
        for i, r in enumerate(runs):
            if _is_embed_run(r[2]):
                e = np.ascontiguousarray(r[2], np.float32)
                if e.shape[1] != dim:
                    raise LmrsError(f"run {i}: embedding rows hold {e.shape[1]} floats, the model's dim is {dim}")
                n.append(e.shape[0]); kind.append(1); embs.append(e.reshape(-1))
            else:
                t = np.ascontiguousarray(r[2], np.uint32).reshape(-1)
                n.append(t.size); kind.append(0); toks.append(t)
        t = np.concatenate(toks) if toks else np.empty(0, np.uint32)
        e = np.concatenate(embs) if embs else np.empty(0, np.float32)
        return np.array(n, np.uint32), np.array(kind, np.uint32), t, e

    def fork(self, src: int, dst: int, n_pos: int) -> None:
        """K/V rows [0, n_pos) of slot `src` (BATCH_CTX: the model's own cache) -> slot `dst` (lmrs_batch_fork)"""
        _chk(lib().lmrs_batch_fork(self._h, src, dst, n_pos))

    @staticmethod
    def _rows(slots, tokens, pos):
        s, t, p = (np.ascontiguousarray(x, np.uint32).reshape(-1) for x in (slots, tokens, pos))
        if not s.size == t.size == p.size:
            raise LmrsError("slots, tokens and pos must have one entry per row")
        return s, t, p

    def forward(self, slots, tokens, pos, logits: bool = False):
        """One pass: row i = forward(tokens[i], pos[i]) on slot slots[i] -> argmax uint32 [n] (and the logits float32 [n, vocab_size] if asked)
        (lmrs_batch_forward)"""
        s, t, p = self._rows(slots, tokens, pos)
        am = np.empty(s.size, np.uint32)
        lg = np.empty((s.size, self.model.args.vocab_size), np.float32) if logits else None
        _chk(lib().lmrs_batch_forward(self._h, s.size, _p(s), _p(t), _p(p), _p(am), _p(lg) if logits else None))
        return (am, lg) if logits else am

    def forward_sample(self, slots, tokens, pos, samplers):
        """One pass, then Sampler.sample per row ON THE DEVICE: row i = forward(tokens[i], pos[i]) on slot slots[i], sampled with samplers[i] (one
        Sampler per row; rows may mix argmax, sample_mult and top-p samplers; a top-p sampler in at most one row) -> next uint32 [n], bit for bit
        Transformer.forward_sample's token for that sampler on a model that holds only that sequence (lmrs_batch_forward_sample)"""
        s, t, p = self._rows(slots, tokens, pos)
        if len(samplers) != s.size:
            raise LmrsError("slots, tokens, pos and samplers must have one entry per row")
        hs = (C.c_void_p * max(s.size, 1))(*[None if x is None else x._h for x in samplers])
        nxt = np.empty(s.size, np.uint32)
        _chk(lib().lmrs_batch_forward_sample(self._h, s.size, _p(s), _p(t), _p(p), C.cast(hs, C.c_void_p), _p(nxt)))
        return nxt

    def forward_runs(self, runs, k: int = 0, logits: bool = False):
        """One pass over runs = [(slot, start_pos, tokens, n_out), ...]: run i feeds its tokens at start_pos .. of its slot (a prompt chunk, a draft, one
        decode row; a slot in at most one run, at most 512 tokens in all) and returns outputs for its LAST n_out rows, packed in run order: argmax uint32 [O];
        with logits also float32 [O, vocab_size]; with k > 0 also topk_idx uint32 [O, k] and topk_logprob float32 [O, k] as score_tokens_topk defines
        them -> argmax, or the tuple (argmax[, logits][, topk_idx, topk_logprob])  (lmrs_batch_forward_runs)
        A run's `tokens` may be a 2-D float32 array [rows, dim] instead: embedding rows, each taken as fill_kv_cache(row, 1, its position) takes it
        (image features beside decode rows); a call with such a run goes through lmrs_batch_forward_runs_embed"""
        if any(_is_embed_run(r[2]) for r in runs):
            s, p, no = (np.array([r[i] for r in runs], np.uint32) for i in (0, 1, 3))
            n, kind, t, e = self._run_rows(runs)
            O, V = int(no.astype(np.int64).sum()), self.model.args.vocab_size
            am = np.empty(O, np.uint32)
            lg = np.empty((O, V), np.float32) if logits else None
            ti, tl = (np.empty((O, k), np.uint32), np.empty((O, k), np.float32)) if k else (None, None)
            _chk(lib().lmrs_batch_forward_runs_embed(self._h, len(runs), _p(s), _p(p), _p(n), _p(no), _p(kind), _p(t) if t.size else None, _p(e),
                                                     _p(am) if O else None, _p(lg) if logits else None, k, _p(ti) if k else None, _p(tl) if k else None))
            out = (am,) + ((lg,) if logits else ()) + ((ti, tl) if k else ())
            return out if len(out) > 1 else am
        toks = [np.ascontiguousarray(r[2], np.uint32).reshape(-1) for r in runs]
        s, p, no = (np.array([r[i] for r in runs], np.uint32) for i in (0, 1, 3))
        n = np.array([t.size for t in toks], np.uint32)
        t = np.concatenate(toks) if toks else np.empty(0, np.uint32)
        O, V = int(no.astype(np.int64).sum()), self.model.args.vocab_size
        am = np.empty(O, np.uint32)
        lg = np.empty((O, V), np.float32) if logits else None
        ti, tl = (np.empty((O, k), np.uint32), np.empty((O, k), np.float32)) if k else (None, None)
        _chk(lib().lmrs_batch_forward_runs(self._h, len(runs), _p(s), _p(p), _p(n), _p(no), _p(t), _p(am) if O else None, _p(lg) if logits else None,
                                           k, _p(ti) if k else None, _p(tl) if k else None))
        out = (am,) + ((lg,) if logits else ()) + ((ti, tl) if k else ())
        return out if len(out) > 1 else am

    def forward_runs_sample(self, runs):
        """forward_runs' pass over runs = [(slot, start_pos, tokens, sampler_or_None), ...] with the LAST row of every run that has a Sampler sampled
        ON THE DEVICE with it; None: the run leaves its K/V rows only (a prompt chunk that is not the last).  Up to `width` runs, 512 tokens in all; runs
        may mix argmax, sample_mult and top-p samplers, a top-p sampler in at most one run -> next uint32 [n_runs] (0 for a None entry), bit for bit
        Transformer.forward_sample's token for that sampler after the run's tokens on a model that holds only that sequence
        (lmrs_batch_forward_runs_sample).  A run's `tokens` may be a 2-D float32 array of embedding rows, as in forward_runs
        (lmrs_batch_forward_runs_embed_sample)"""
        if any(_is_embed_run(r[2]) for r in runs):
            s, p = (np.array([r[i] for r in runs], np.uint32) for i in (0, 1))
            n, kind, t, e = self._run_rows(runs)
            hs = (C.c_void_p * max(len(runs), 1))(*[None if r[3] is None else r[3]._h for r in runs])
            nxt = np.zeros(len(runs), np.uint32)
            _chk(lib().lmrs_batch_forward_runs_embed_sample(self._h, len(runs), _p(s), _p(p), _p(n), _p(kind), _p(t) if t.size else None, _p(e),
                                                            C.cast(hs, C.c_void_p), _p(nxt)))
            return nxt
        toks = [np.ascontiguousarray(r[2], np.uint32).reshape(-1) for r in runs]
        s, p = (np.array([r[i] for r in runs], np.uint32) for i in (0, 1))
        n = np.array([t.size for t in toks], np.uint32)
        t = np.concatenate(toks) if toks else np.empty(0, np.uint32)
        hs = (C.c_void_p * max(len(runs), 1))(*[None if r[3] is None else r[3]._h for r in runs])
        nxt = np.zeros(len(runs), np.uint32)
        _chk(lib().lmrs_batch_forward_runs_sample(self._h, len(runs), _p(s), _p(p), _p(n), _p(t), C.cast(hs, C.c_void_p), _p(nxt)))
        return nxt

    def generate_greedy(self, slots, tokens, pos, n_new: int, timing: bool = False):
        """n_new greedy steps of every row on the device -> uint32 [n, n_new]: row i = Transformer.generate_greedy([tokens[i]], n_new, pos[i]) on its
        slot (and device seconds if timing) (lmrs_batch_generate_greedy)"""
        s, t, p = self._rows(slots, tokens, pos)
        out = np.zeros((s.size, n_new), np.uint32); sec = C.c_double()
        _chk(lib().lmrs_batch_generate_greedy(self._h, s.size, _p(s), _p(t), _p(p), n_new, _p(out), C.byref(sec)))
        return (out, sec.value) if timing else out

    def generate_topp(self, slots, tokens, pos, max_new, stop=None, samplers=None, check_every: int = 4, logprobs: bool = False, timing: bool = False):
        """generate with top-p samplers admitted (each in one row only): their candidate vectors live on the device for the length of the call and are
        back in the samplers when it returns, so whatever is done with a sampler next continues exactly.  A row whose step finds no candidate above the
        cutoff ends with finish FINISH_NO_CANDIDATE and reports no token for that step.  Arguments and results as generate  (lmrs_batch_generate_topp)"""
        return self.generate(slots, tokens, pos, max_new, stop, samplers, check_every, logprobs, timing, _call="lmrs_batch_generate_topp")

    def generate(self, slots, tokens, pos, max_new, stop=None, samplers=None, check_every: int = 4, logprobs: bool = False, timing: bool = False, *,
                 _call: str = "lmrs_batch_generate"):
        """The device loop whose rows end one by one: row i feeds tokens[i] at pos[i] of slots[i] and goes on with what it chose - Sampler.sample with
        samplers[i], the argmax for None (samplers=None: every row) - until it chooses a token of its stop set (finish STOP; the token is reported, never
        fed) or has produced max_new[i] tokens (BUDGET).  max_new: one budget per row, or a scalar for all.  stop: a list of token lists, one per row, or
        one list of tokens for all rows; at most STOP_MAX tokens a row.  Samplers: argmax and sample_mult ones (top-p is refused); they may be shared.
        check_every: passes between two looks at the rows' state - the results do not depend on it.
        -> (tokens, finish[, logprobs], stats): tokens a list of uint32 arrays, row i cut to its n_out; finish uint32 [n] (FINISH_BUDGET /
        FINISH_STOP, FINISH_FINAL where the row's slot has an automaton that reached a final state); logprobs a list of float32 arrays of the same lengths - log softmax of the row each token was chosen from, at that token; stats a
        dict: passes, row_passes (and seconds, host wall time, if timing)  (lmrs_batch_generate)"""
        s, t, p = self._rows(slots, tokens, pos)
        n = s.size
        mx = np.asarray(max_new)
        mx = np.ascontiguousarray(np.full(n, mx) if mx.ndim == 0 else mx.reshape(-1), np.uint32)
        if mx.size != n:
            raise LmrsError("max_new must be a scalar or hold one budget per row")
        ns, st = None, None
        if stop is not None:
            sets = list(stop)
            if not (len(sets) == n and all(hasattr(x, "__len__") for x in sets)):     # one list for all rows
                if any(hasattr(x, "__len__") for x in sets):
                    raise LmrsError("stop must be one list of tokens, or one list of tokens per row")
                sets = [sets] * n
            ns = np.array([len(x) for x in sets], np.uint32)
            st = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32).reshape(-1) for x in sets]) if n else [], np.uint32)
        if samplers is not None and len(samplers) != n:
            raise LmrsError("samplers must have one entry per row (None: the argmax)")
        hs = None if samplers is None else (C.c_void_p * max(n, 1))(*[None if x is None else x._h for x in samplers])
        M = int(mx.max()) if n else 0
        out = np.zeros((n, max(M, 1)), np.uint32)
        lp = np.zeros((n, max(M, 1)), np.float32) if logprobs else None
        n_out, fin = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        stats2, sec = np.zeros(2, np.uint64), C.c_double()
        _chk(getattr(lib(), _call)(self._h, n, _p(s), _p(t), _p(p), _p(mx), None if ns is None else _p(ns), _p(st) if st is not None and st.size else None,
                                   None if hs is None else C.cast(hs, C.c_void_p), check_every, _p(out), _p(lp) if logprobs else None, _p(n_out), _p(fin),
                                   _p(stats2), C.byref(sec)))
        stats = dict(passes=int(stats2[0]), row_passes=int(stats2[1]))
        if timing:
            stats["seconds"] = sec.value
        toks = [out[i, :n_out[i]].copy() for i in range(n)]
        res = (toks, fin) + (([lp[i, :n_out[i]].copy() for i in range(n)],) if logprobs else ()) + (stats,)
        return res

    def kv_row(self, slot: int, which: int, layer: int, pos: int) -> np.ndarray:
        """Transformer.kv_row of `slot`'s cache (lmrs_batch_debug_kv)"""
        out = np.empty(self.model.args.n_kv_heads * self.model.args.head_size, np.float32)
        _chk(lib().lmrs_batch_debug_kv(self._h, slot, which, layer, pos, _p(out)))
        return out

    debug_kv = kv_row


def shard_plan(args: TransformerArgs, rank: int, world: int) -> dict:
    """Row ranges (first, count) shard `rank` of `world` owns; host-only."""
    p = (C.c_int * 10)()
    _chk(lib().lmrs_shard_plan(C.byref(args), rank, world, p))
    k = ["q_heads", "kv_heads", "dim_rows", "hidden_pairs", "vocab_rows"]
    return {k[i]: (p[2 * i], p[2 * i + 1]) for i in range(5)}


def comm_unique_id() -> bytes:
    """128-byte ncclUniqueId for Transformer(..., world > 1): make it on rank 0, broadcast it to the other ranks."""
    buf = C.create_string_buffer(128)
    _chk(lib().lmrs_comm_unique_id(buf))
    return buf.raw


class ShardGroup:
    """`world` row shards of one model on ONE device (verification aid: the multi-GPU partitioning without RCCL)."""

    def __init__(self, data, world: int, device: int = 0):
        image = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8)
        self._arr = (C.c_void_p * world)()
        used = C.c_size_t()
        _chk(lib().lmrs_group_create(_p(image), image.size, device, world, self._arr, C.byref(used)))
        self.world = world
        self.args = lib().lmrs_get_args(self._arr[0]).contents

    def forward(self, token: int, pos: int):
        p, n = C.POINTER(C.c_float)(), C.c_uint32()
        _chk(lib().lmrs_group_forward(self._arr, self.world, token, pos, C.byref(p), C.byref(n)))
        return np.ctypeslib.as_array(p, shape=(self.args.vocab_size,)), n.value

    def close(self):
        for i in range(self.world):
            if self._arr[i]:
                lib().lmrs_destroy(self._arr[i]); self._arr[i] = None

    __del__ = close


# ---- free functions (functional.rs / quantization.rs), each on the device kernels
def matmul_q8(xq, xs, wq, ws, n, o, gs=128, sl=1, device=0):
    out = np.zeros(sl * o, np.float32)
    _chk(lib().lmrs_op_matmul_q8(device, _p(out), _p(np.ascontiguousarray(xq, np.int8)), _p(np.ascontiguousarray(xs, np.float32)),
                                 _p(np.ascontiguousarray(wq, np.int8)), _p(np.ascontiguousarray(ws, np.float32)), n, o, gs, sl))
    return out


def w13_quant(xq, xs, wq, ws, n, o, n_tok, gemma=False, device=0):
    """The batched w1/w3 projection with the activation and the next matmul's quantiser in its epilogue (lmrs_debug_w13_quant):
    -> (n_tok x o/2 int8, n_tok x o/256 scales)."""
    hq = np.empty(n_tok * (o // 2), np.int8); hs = np.empty(n_tok * (o // 256), np.float32)
    _chk(lib().lmrs_debug_w13_quant(device, _p(hq), _p(hs), _p(np.ascontiguousarray(xq, np.int8)), _p(np.ascontiguousarray(xs, np.float32)),
                                    _p(np.ascontiguousarray(wq, np.int8)), _p(np.ascontiguousarray(ws, np.float32)), n, o, n_tok, int(bool(gemma))))
    return hq, hs


def matmul_q4(xq, xs, wq, ws, n, o, gs=128, device=0):
    out = np.zeros(o, np.float32)
    _chk(lib().lmrs_op_matmul_q4(device, _p(out), _p(np.ascontiguousarray(xq, np.uint8)), _p(np.ascontiguousarray(xs, np.float32)),
                                 _p(np.ascontiguousarray(wq, np.uint8)), _p(np.ascontiguousarray(ws, np.float32)), n, o, gs))
    return out


def quantize(x, gs=128, device=0):
    x = np.ascontiguousarray(x, np.float32)
    q = np.empty(x.size, np.int8); s = np.empty(x.size // gs, np.float32)
    _chk(lib().lmrs_op_quantize(device, _p(q), _p(s), _p(x), x.size, gs))
    return q, s


def quantize_q4(x, gs=128, device=0):
    x = np.ascontiguousarray(x, np.float32)
    q = np.empty(x.size // 2, np.uint8); s = np.empty(x.size // gs, np.float32)
    _chk(lib().lmrs_op_quantize_q4(device, _p(q), _p(s), _p(x), x.size, gs))
    return q, s


def rmsnorm(x, w, eps, add_unit_offset=False, device=0):
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
    o = np.empty_like(x)
    _chk(lib().lmrs_op_rmsnorm(device, _p(o), _p(x), _p(w), x.size, eps, int(add_unit_offset)))
    return o


def softmax(x, device=0):
    x = np.array(x, np.float32, copy=True)
    _chk(lib().lmrs_op_softmax(device, _p(x), x.size))
    return x


def topk(logits, k: int, written=None, device=0):
    """The selection kernels of score_topk / forward_topk on one row: `logits` holds the first `written` (default: all) of n = len(logits)
    entries, the rest count as 0.0 -> (idx uint32 [k], values float32 [k]) in rank order (lmrs_op_topk)."""
    lg = np.ascontiguousarray(logits, np.float32)
    idx = np.empty(max(int(k), 0), np.uint32); val = np.empty(idx.size, np.float32)
    _chk(lib().lmrs_op_topk(device, _p(lg), lg.size, lg.size if written is None else written, k, _p(idx), _p(val)))
    return idx, val


def classifier_argmax(x, rms_w, wq, ws, eps, device=0):
    """Final rmsnorm + quantize + matmul_q8 (transformer.rs:341-381) + sample_argmax (sampler.rs:29-41) -> (token, logits)."""
    x = np.ascontiguousarray(x, np.float32); rms_w = np.ascontiguousarray(rms_w, np.float32)
    wq = np.ascontiguousarray(wq, np.int8); ws = np.ascontiguousarray(ws, np.float32)
    n = x.size; o = wq.size // n
    tok = C.c_uint32(); logits = np.empty(o, np.float32)
    _chk(lib().lmrs_op_classifier_argmax(device, _p(x), _p(rms_w), _p(wq), _p(ws), n, o, eps, C.byref(tok), _p(logits)))
    return tok.value, logits


def expf(x, device=0):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    _chk(lib().lmrs_op_expf(device, _p(y), _p(x), x.size))
    return y


def sample_mult(logits, temperature: float, rnd: float, device=0):
    """Sampler::sample (temperature != 0, sample_mult) on the device -> (token, the probabilities the logits were turned into)"""
    lg = np.ascontiguousarray(logits, np.float32).copy()
    tok = C.c_uint32()
    _chk(lib().lmrs_op_sample_mult(device, _p(lg), lg.size, C.c_float(temperature), C.c_float(rnd), C.byref(tok)))
    return tok.value, lg


def op_sample_rows(rows, temperature, top_p, rnd, pairs: bool = True, device=0):
    """Sampler::sample on the device for up to 16 rows of logits at once, row r with temperature[r], top_p[r] and the random number rnd[r]
    (lmrs_op_sample_rows) -> (probabilities float32 [n_rows, n] - rows of temperature 0 untouched -, token uint32 [n_rows] of the sample_mult rows,
    n0 uint32 [n_rows] of the top-p rows, and with pairs a list of the top-p rows' candidates (prob float32 [n0], index uint32 [n0]) in index order)"""
    x = np.ascontiguousarray(rows, np.float32).copy()
    if x.ndim != 2:
        raise LmrsError("op_sample_rows: rows must be [n_rows, n]")
    t, p, r = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (temperature, top_p, rnd))
    if not t.size == p.size == r.size == x.shape[0]:
        raise LmrsError("op_sample_rows: one temperature, top_p and rnd per row")
    tok, n0 = np.zeros(x.shape[0], np.uint32), np.zeros(x.shape[0], np.uint32)
    pr = np.zeros(x.shape, dtype=[("prob", np.float32), ("index", np.uint32)]) if pairs else None
    _chk(lib().lmrs_op_sample_rows(device, _p(x), x.shape[0], x.shape[1], _p(t), _p(p), _p(r), _p(tok), _p(n0), _p(pr) if pairs else None))
    if not pairs:
        return x, tok, n0
    return x, tok, n0, [(pr[i, : n0[i]]["prob"].copy(), pr[i, : n0[i]]["index"].copy()) for i in range(x.shape[0])]


PAIR = np.dtype([("prob", np.float32), ("index", np.uint32)])


def op_sort_candidates(pairs, n0, device=0):
    """The device sort of forward_runs_sample's flat top-p rows on caller-supplied candidates, all rows in one call of its launcher: pairs [n_rows, ld]
    of PAIR (prob >= 0), the first n0[r] of row r in ascending index order -> a copy whose row r has its first n0[r] entries by descending prob, ties by
    ascending index; everything else as it was (lmrs_op_sort_candidates)"""
    x = np.ascontiguousarray(pairs, PAIR)
    if x.ndim != 2:
        raise LmrsError("op_sort_candidates: pairs must be [n_rows, ld]")
    n = np.ascontiguousarray(n0, np.uint32).reshape(-1)
    if n.size != x.shape[0]:
        raise LmrsError("op_sort_candidates: one n0 per row")
    out = x.copy()
    _chk(lib().lmrs_op_sort_candidates(device, _p(x), x.shape[0], x.shape[1], _p(n), _p(out)))
    return out


def op_topp_rows(cand, n0, top_p, rnd, state, device=0):
    """The launches that finish generate_topp's top-p rows, on caller-supplied rows: cand [n_rows, n] of PAIR, the first n0[r] of row r the call's
    candidates in ascending index order; state [n_rows, n] of PAIR, each row a persistent vector in descending order of prob; top_p, rnd per row
    -> (token [n_rows], status [n_rows]: 0 a token, 1 no candidate, new state)  (lmrs_op_topp_rows)"""
    x = np.ascontiguousarray(cand, PAIR)
    st = np.array(state, PAIR, order="C")
    if x.ndim != 2 or st.shape != x.shape:
        raise LmrsError("op_topp_rows: cand and state must both be [n_rows, n]")
    n = np.ascontiguousarray(n0, np.uint32).reshape(-1)
    tp = np.ascontiguousarray(top_p, np.float32).reshape(-1); rn = np.ascontiguousarray(rnd, np.float32).reshape(-1)
    if not n.size == tp.size == rn.size == x.shape[0]:
        raise LmrsError("op_topp_rows: one n0, top_p and rnd per row")
    tok = np.zeros(x.shape[0], np.uint32); status = np.zeros(x.shape[0], np.uint32)
    _chk(lib().lmrs_op_topp_rows(device, x.shape[0], x.shape[1], _p(x), _p(n), _p(tp), _p(rn), _p(st), _p(tok), _p(status)))
    return tok, status, st


def bench_topp_rows(n_rows: int, n: int, n0: int, iters: int = 5, device=0):
    """(device microseconds of the launches behind op_topp_rows on n_rows rows of n0 candidates over vectors of n entries, mean of iters runs; how many
    launches a run has)  (lmrs_bench_topp_rows)"""
    us = C.c_double(); k = C.c_int()
    _chk(lib().lmrs_bench_topp_rows(device, n_rows, n, n0, iters, C.byref(us), C.byref(k)))
    return us.value, k.value


def bench_sample_rows(n_rows: int, n: int, iters: int = 5, device=0):
    """device microseconds per run of the six launches behind op_sample_rows with both chains walking all n terms, and the nominal shader clock in MHz
    (lmrs_bench_sample_rows)"""
    us = np.zeros(6, np.float64); mhz = C.c_double()
    _chk(lib().lmrs_bench_sample_rows(device, n_rows, n, iters, _p(us), C.byref(mhz)))
    return us / iters, mhz.value


def tanh_cast(x, c=1.0, device=0):
    """(float)tanh(c * (double)x) as the kernels evaluate it (Gemma soft-caps: c = 1; tanh-GELU: c = 0.7978845608028654)"""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    _chk(lib().lmrs_op_tanh_cast(device, _p(y), _p(x), x.size, float(c)))
    return y


class VisionTransformer:
    """lmrs::vision::VisionTransformer (src/vision.rs): the CLIP image tower of the multimodal models, on the device."""

    def __init__(self, section: np.ndarray, device: int = 0):
        sec = np.ascontiguousarray(section, np.uint8)
        h = C.c_void_p(); used = C.c_size_t()
        _chk(lib().lmrs_vision_create(sec.ctypes.data, sec.size, device, C.byref(h), C.byref(used)))
        self._h, self.bytes_consumed = h, used.value

    def forward(self, pixel_values: np.ndarray, num_crops: int) -> np.ndarray:
        """-> float32 [num_crops, 576, dim] (vision.rs:244-577; the class token is dropped)."""
        pv = np.ascontiguousarray(pixel_values, np.float32).reshape(-1)
        if pv.size != num_crops * 3 * 336 * 336:
            raise LmrsError("pixel_values must hold num_crops * 3 * 336 * 336 floats")
        out = np.empty(num_crops * 576 * 1024, np.float32); ns = C.c_uint32()
        _chk(lib().lmrs_vision_forward(self._h, pv.ctypes.data, num_crops, out.ctypes.data, C.byref(ns)))
        return out.reshape(num_crops, 576, ns.value // 576)

    def close(self):
        if self._h:
            lib().lmrs_vision_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rope_terms(model_type: int, rope_theta: float, head_size: int, pos: int, j: int):
    """(cos, sin) of the RoPE table lmrs_create builds, for one position and pair index (host-only, no GPU)."""
    a = TransformerArgs(); a.model_type = model_type; a.rope_theta = rope_theta; a.head_size = head_size
    c, s_ = C.c_float(), C.c_float()
    _chk(lib().lmrs_rope_terms(C.byref(a), pos, j, C.byref(c), C.byref(s_)))
    return np.float32(c.value), np.float32(s_.value)


def draft_lookup(hist, ngram_max: int, max_draft: int) -> np.ndarray:
    """Prompt-lookup drafting, host only: the tokens that followed the latest earlier occurrence of the longest suffix of `hist` of at most
    ngram_max tokens, at most max_draft of them (empty: no match) (lmrs_draft_lookup)."""
    h = np.ascontiguousarray(hist, np.uint32).reshape(-1)
    d = np.zeros(max(int(max_draft), 1), np.uint32); n = C.c_uint32()
    _chk(lib().lmrs_draft_lookup(_p(h), h.size, ngram_max, max_draft, _p(d), C.byref(n)))
    return d[:n.value].copy()


def debug_gemm_wide(xq, xs, wq, ws, n: int, o: int, n_tok: int, q4: bool = False, device: int = 0) -> np.ndarray:
    """The stream GEMM of a 17 .. 47-row batch pass on caller-supplied operands, here at any 1 <= n_tok <= 64 -> float32 [n_tok, o] (lmrs_debug_gemm_wide)."""
    xq = np.ascontiguousarray(xq); xs = np.ascontiguousarray(xs, np.float32); wq = np.ascontiguousarray(wq); ws = np.ascontiguousarray(ws, np.float32)
    out = np.empty((n_tok, o), np.float32)
    _chk(lib().lmrs_debug_gemm_wide(device, _p(out), _p(xq), _p(xs), _p(wq), _p(ws), n, o, n_tok, int(bool(q4))))
    return out


def debug_gemm_skinny(xq, xs, wq, ws, n: int, o: int, n_tok: int, q4: bool = False, device: int = 0) -> np.ndarray:
    """The skinny GEMM of verify_tokens' pass on caller-supplied operands -> float32 [n_tok, o] (lmrs_debug_gemm_skinny)."""
    xq = np.ascontiguousarray(xq); xs = np.ascontiguousarray(xs, np.float32); wq = np.ascontiguousarray(wq); ws = np.ascontiguousarray(ws, np.float32)
    out = np.empty((n_tok, o), np.float32)
    _chk(lib().lmrs_debug_gemm_skinny(device, _p(out), _p(xq), _p(xs), _p(wq), _p(ws), n, o, n_tok, int(bool(q4))))
    return out


def gemm_tile(n: int, o: int, n_tok: int, q4: bool = False):
    """(weight rows, tokens, waves) of the workgroup tile the batched matmul_q8 / matmul_q4 runs this launch with (host arithmetic only, no GPU);
    (0, 0, 0) below 48 tokens: the direct kernels (lmrs_debug_gemm_tile)."""
    tm, tn, w = C.c_int(), C.c_int(), C.c_int()
    _chk(lib().lmrs_debug_gemm_tile(n, o, n_tok, int(bool(q4)), C.byref(tm), C.byref(tn), C.byref(w)))
    return tm.value, tn.value, w.value


def processor_hd_transform(out_patches: np.ndarray, w_crop: int, h_crop: int, glb_gn: np.ndarray, sub_gn: np.ndarray) -> np.ndarray:
    """Host-only: the projector's input rows (processor.rs:240-254, 377-418, 480-484) -> float32 [n_embeds, 4096]."""
    op = np.ascontiguousarray(out_patches, np.float32).reshape(-1)
    g = np.ascontiguousarray(glb_gn, np.float32).reshape(-1); s_ = np.ascontiguousarray(sub_gn, np.float32).reshape(-1)
    ne = (h_crop * 12) * (w_crop * 12 + 1) + 12 * 13 + 1
    out = np.empty(ne * 4096, np.float32); n = C.c_uint32()
    _chk(lib().lmrs_processor_hd_transform(op.ctypes.data, op.size, 576 * 1024, w_crop, h_crop, g.ctypes.data, s_.ctypes.data, out.ctypes.data, C.byref(n)))
    return out[: n.value * 4096].reshape(n.value, 4096)


class PHI3VProcessor:
    """lmrs::processor::PHI3VProcessor (src/processor.rs:168-342): HD transform + two-layer projector, on the device."""

    def __init__(self, section: np.ndarray, device: int = 0):
        sec = np.ascontiguousarray(section, np.uint8)
        h = C.c_void_p(); used = C.c_size_t()
        _chk(lib().lmrs_processor_create(sec.ctypes.data, sec.size, device, C.byref(h), C.byref(used)))
        self._h, self.bytes_consumed = h, used.value
        self.text_dim = int(np.frombuffer(sec[4:8].tobytes(), np.uint32)[0])

    def forward(self, out_patches: np.ndarray, new_shape: int, patch_side: int, w_crop: int, h_crop: int) -> np.ndarray:
        """-> float32 [num_embeds, text_dim] (processor.rs:234-342)."""
        op = np.ascontiguousarray(out_patches, np.float32).reshape(-1)
        ne = (h_crop * patch_side) * (w_crop * patch_side + 1) + patch_side * (patch_side + 1) + 1
        out = np.empty(ne * self.text_dim, np.float32); n = C.c_uint32()
        _chk(lib().lmrs_processor_forward(self._h, op.ctypes.data, op.size, new_shape, patch_side, w_crop, h_crop, out.ctypes.data, C.byref(n)))
        return out[: n.value * self.text_dim].reshape(n.value, self.text_dim)

    def close(self):
        if self._h:
            lib().lmrs_processor_destroy(self._h); self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tokenizer:
    """lmrs::tokenizer::Tokenizer (reference src/tokenizer.rs): Tokenizer(path or bytes), .bos / .eos, encode(), decode().  Host code."""

    def __init__(self, src):
        data = open(src, "rb").read() if isinstance(src, str) else bytes(src)
        buf = np.frombuffer(data, np.uint8)
        h = C.c_void_p()
        _chk(lib().lmrs_tokenizer_create(_p(buf), buf.size, C.byref(h)))
        self._h = h
        v, b, e = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _chk(lib().lmrs_tokenizer_info(h, C.byref(v), C.byref(b), C.byref(e)))
        self.vocab_size, self.bos, self.eos = v.value, b.value, e.value

    def encode(self, text: str, bos: bool, eos: bool, chat_format: bool, model_type: int) -> np.ndarray:
        raw = text.encode("utf-8")
        out = np.empty(len(raw) + 32, np.uint32); n = C.c_size_t()
        _chk(lib().lmrs_tokenizer_encode(self._h, raw, len(raw), int(bos), int(eos), int(chat_format), int(model_type), _p(out), out.size, C.byref(n)))
        return out[: n.value].copy()

    def decode(self, token: int) -> str:
        buf = C.create_string_buffer(256); n = C.c_size_t()
        _chk(lib().lmrs_tokenizer_decode(self._h, token, buf, 256, C.byref(n)))
        return buf.raw[: n.value].decode("utf-8")

    def close(self):
        if getattr(self, "_h", None):
            lib().lmrs_tokenizer_destroy(self._h); self._h = None

    __del__ = close


class Sampler:
    """lmrs::sampler::Sampler (reference src/sampler.rs): Sampler(vocab_size, temperature, top_p, seed).sample(logits).  Host code;
    `logits` (float32, C-contiguous) is modified in place when temperature != 0, as in the reference."""

    def __init__(self, vocab_size: int, temperature: float, top_p: float, seed: int):
        h = C.c_void_p()
        _chk(lib().lmrs_sampler_create(vocab_size, temperature, top_p, seed, C.byref(h)))
        self._h, self.vocab_size = h, vocab_size

    def sample(self, logits: np.ndarray) -> int:
        assert logits.dtype == np.float32 and logits.flags.c_contiguous and logits.size >= self.vocab_size
        nxt = C.c_uint32()
        _chk(lib().lmrs_sampler_sample(self._h, _p(logits), C.byref(nxt)))
        return nxt.value

    def sample_exps(self, exps: np.ndarray) -> int:
        """Sampler::sample from the softmax's exponentials on (lmrs_sampler_sample_exps): exps = exp(logits / temperature - max), turned into the probabilities in place"""
        assert exps.dtype == np.float32 and exps.flags.c_contiguous and exps.size >= self.vocab_size
        nxt = C.c_uint32()
        _chk(lib().lmrs_sampler_sample_exps(self._h, _p(exps), C.byref(nxt)))
        return nxt.value

    def topp_pairs(self, prob: np.ndarray, index: np.ndarray) -> int:
        """sample_topp from its sort on: the candidates (prob >= cutoff, in index order) were filtered elsewhere (lmrs_sampler_topp_pairs)"""
        pairs = np.zeros(prob.size, dtype=[("prob", np.float32), ("index", np.uint32)])
        pairs["prob"] = prob; pairs["index"] = index
        nxt = C.c_uint32()
        _chk(lib().lmrs_sampler_topp_pairs(self._h, _p(pairs) if prob.size else None, prob.size, C.byref(nxt)))
        return nxt.value

    def topp_sorted_pairs(self, prob: np.ndarray, index: np.ndarray) -> int:
        """topp_pairs for candidates the caller has also sorted, by descending prob, ties in index order (lmrs_sampler_topp_sorted_pairs)"""
        pairs = np.zeros(prob.size, dtype=[("prob", np.float32), ("index", np.uint32)])
        pairs["prob"] = prob; pairs["index"] = index
        nxt = C.c_uint32()
        _chk(lib().lmrs_sampler_topp_sorted_pairs(self._h, _p(pairs) if prob.size else None, prob.size, C.byref(nxt)))
        return nxt.value

    def candidates(self):
        """(the persistent candidate vector as it stands, a PAIR array of vocab_size entries; whether it is known to be in descending order of prob)
        (lmrs_sampler_candidates)"""
        pairs = np.zeros(self.vocab_size, PAIR); ordered = C.c_int()
        _chk(lib().lmrs_sampler_candidates(self._h, _p(pairs), C.byref(ordered)))
        return pairs, bool(ordered.value)

    def set_candidates(self, pairs) -> None:
        """replace the persistent vector (vocab_size PAIR entries); the order flag follows from what is given  (lmrs_sampler_set_candidates)"""
        x = np.ascontiguousarray(pairs, PAIR).reshape(-1)
        if x.size != self.vocab_size:
            raise LmrsError("set_candidates: the vector has vocab_size = %d entries, %d were given" % (self.vocab_size, x.size))
        _chk(lib().lmrs_sampler_set_candidates(self._h, _p(x)))

    def info(self):
        """(vocab_size, temperature, top_p, the random number every call draws: random_f32(seed), sampler.rs:119)"""
        v = C.c_uint32(); t = C.c_float(); p = C.c_float(); r = C.c_float()
        _chk(lib().lmrs_sampler_info(self._h, C.byref(v), C.byref(t), C.byref(p), C.byref(r)))
        return v.value, t.value, p.value, r.value

    def close(self):
        if getattr(self, "_h", None):
            lib().lmrs_sampler_destroy(self._h); self._h = None

    __del__ = close


def min_p_gap(min_p: float, temperature: float = 1.0) -> np.float32:
    """The min_gap of Batch.set_filters that keeps the tokens whose probability at `temperature` is at least min_p times the largest:
    -temperature * ln(min_p), formed in float64 and rounded once to float32.  min_p <= 0: inf (off); temperature 0 (argmax rows): 0"""
    if not (min_p <= 1.0) or not (temperature >= 0.0):
        raise LmrsError("min_p must lie in [0, 1] and temperature must not be negative")
    if min_p <= 0.0:
        return np.float32(np.inf)
    return np.float32(-np.float64(temperature) * np.log(np.float64(min_p)) + 0.0)


def filter_rows(rows, top_k=0, min_gap=float("inf"), n=None, device: int = 0) -> np.ndarray:
    """The filter kernel alone over rows (float32 [n_rows, ld]; n: the logits a row holds, default ld): a copy with top_k / min_gap (a scalar, or one value
    per row; (0, inf): the row is left alone) applied by the rule of include/lmrs_hip.h; columns from n on come back as they went (lmrs_op_filter_rows)"""
    x = np.array(rows, np.float32, ndmin=2, order="C")
    k = np.ascontiguousarray(np.broadcast_to(np.asarray(top_k, np.uint32), (x.shape[0],)))
    g = np.ascontiguousarray(np.broadcast_to(np.asarray(min_gap, np.float32), (x.shape[0],)))
    _chk(lib().lmrs_op_filter_rows(device, _p(x), x.shape[0], x.shape[1] if n is None else n, x.shape[1], _p(k), _p(g)))
    return x


def automaton_masks(ta: TokenAutomaton, device: int = 0) -> np.ndarray:
    """The per-state masks of `ta` as the device builds them -> uint32 [n_states, W] in pack_mask's layout (lmrs_op_automaton_masks)"""
    out = np.zeros((ta.n_states, (ta.vocab_size + 31) // 32), np.uint32)
    _chk(lib().lmrs_op_automaton_masks(device, ta.vocab_size, ta.n_states, ta.n_classes, _p(ta.class_of), _p(ta.next), _p(out)))
    return out
