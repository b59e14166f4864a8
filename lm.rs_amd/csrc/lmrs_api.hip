// lmrs_api.hip — host side of the MI355X decode path and its C ABI (include/lmrs_hip.h).
//
// Mirrors lmrs::transformer::Transformer (reference src/transformer.rs): `new` (:134-314) becomes
// lmrs_create (parse LMRS, upload weights to HBM, allocate KV cache + activations), `forward`
// (:316-384) becomes one replay of a captured hipGraph (embedding -> n_layers x 5 fused kernels ->
// classifier -> argmax), `get_embeddings` (:659-669) and `fill_kv_cache` (:672-684) likewise.
//
// HBM layout (all 256-byte aligned inside one arena):
//   per layer  Wqkv  [(att+2kv) x dim] int8 (wq|wk|wv rows concatenated)  + scales [(att+2kv) x dim/128] f32
//              Wo    [dim x att]                                          + scales
//              W13   [2*hidden x dim], rows interleaved 2i = w1 (gate) row i, 2i+1 = w3 (up) row i
//              W2    [dim x hidden]
//              rms weights f32[dim] (att, post_att, and for Gemma pre_ffn, post_ffn)
//   embedding / classifier table [vocab x dim] (+ Phi lm_head), rms_final
//   KV cache   2 x [n_layers][seq_len][kv_dim] f32  (same layout as the reference, transformer.rs:302-303,413)
//   RoPE table [seq_len][head/2] (fcr, fci) built on the host with libm (transformer.rs:446-482)
//   activations x[dim], q[att], k_raw[kv], att_out[att], h[hidden], logits[vocab], argmax partials,
//   tokens[seq_len+1], DevState
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "../../include/lmrs_hip.h"
#include "lmrs_automaton.h"
#include "lmrs_buf.h"
#include "lmrs_device_math.h"
#include "lmrs_format.h"
#include "lmrs_kernels.h"
#include "lmrs_pages.h"
#include "lmrs_score.h"
#include "lmrs_switches.h"

using namespace lmrs;

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return -1; }
#define HIP_OK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(std::string(#expr) + ": " + hipGetErrorString(e_));            \
    } while (0)

extern "C" const char* lmrs_last_error(void) { return g_err.c_str(); }
// The owners of device and pinned memory (lmrs_buf.h): the only callers of the runtime's free functions in this file besides the arenas and pfx_*
static thread_local hipError_t g_alloc_err = hipSuccess;                       // what the last obtain returned
struct DevMem { static void* obtain(size_t bytes) { void* p = nullptr; return (g_alloc_err = hipMalloc(&p, bytes)) == hipSuccess ? p : nullptr; } static void release(void* p) { (void)hipFree(p); } };
struct PinMem { static void* obtain(size_t bytes) { void* p = nullptr; return (g_alloc_err = hipHostMalloc(&p, bytes, hipHostMallocDefault)) == hipSuccess ? p : nullptr; } static void release(void* p) { (void)hipHostFree(p); } };
template <class T> using DevBuf = Buf<T, DevMem>;
template <class T> using PinBuf = Buf<T, PinMem>;
// the message of an allocation that failed where the call reports the runtime's own error (the others say "out of memory" and clear it)
static int alloc_failed(const char* what) { return fail(std::string(what) + ": " + hipGetErrorString(g_alloc_err)); }
namespace lmrs { int text_fail(const char* msg) { return fail(msg); } }       // lmrs_text.cpp reports through the same message slot

namespace {

struct DevLayer {
    const void *wqkv, *wo, *w13, *w2;
    const float *sqkv, *so, *s13, *s2;
    const float *sqkvT = nullptr, *soT = nullptr, *s13T = nullptr, *s2T = nullptr;    // the same scales TRANSPOSED ([group][row]) for the batched path's ring GEMMs (prefill_alloc)
    const float *rms_att, *rms_post_att, *rms_pre_ffn, *rms_post_ffn;
};

}  // namespace
static int prefill_alloc(lmrs_ctx* c);       // (defined with the batched prefill below; lmrs_create calls it for RCCL row shards)

struct lmrs_ctx {
    lmrs_args args{};
    Layout lay;
    int device = 0;
    hipStream_t stream = nullptr;
    char* arena = nullptr; size_t arena_bytes = 0, arena_used = 0;
    std::vector<DevLayer> layers;
    const void *emb_q = nullptr, *cls_q = nullptr; const float *emb_s = nullptr, *cls_s = nullptr, *rms_final = nullptr;
    float *x = nullptr, *q = nullptr, *k_raw = nullptr, *att_out = nullptr, *h = nullptr, *logits = nullptr, *tmp = nullptr;
    float *part_val = nullptr; int* part_idx = nullptr;
    float *k_cache = nullptr, *v_cache = nullptr, *rope = nullptr;
    float* stage = nullptr; size_t stage_floats = 0;        // device staging for fill_kv_cache / get_embeddings
    uint32_t* tokens = nullptr; DevState* st = nullptr;
    unsigned long long* dbg = nullptr; int dbg_node = 0;     // LMRS_DEBUG_TIMELINE=1: 8 stamps per kernel node
    // pinned host
    DevBuf<unsigned long long> samp_keys; DevBuf<float> samp_pairs; PinBuf<char> h_pairs; int samp_cap = 0;   // lmrs_forward_sample: the device sort of top-p candidates (allocated on first use; samp_cap != 0: the set stands)
    PinBuf<float> h_logits; PinBuf<uint32_t> h_tok; PinBuf<DevState> h_st; unsigned h_st_next = 0;   // h_st: ring of kStateSlots pinned slots (an async copy may still be reading the previous one)
    // the step graphs by form (StepForm: qkv + attention mode 0..2 | 3 + split-attention bucket 0..3 | 7 + bucket: the split form with its scores in the
    // qkv launch) and steps per launch ([0] one, [1] multi_k):
    // step_graph captures a missing one; the graph of position 0's form (primary_graph) is what says "this context replays graphs"
    hipGraphExec_t g_steps[11][2] = {}, g_layers = nullptr;
    // long contexts: from att_split_pos on a step's attention is the split pair (256-key chunks: 4, 8, 16, 32 by context bucket), scores in att_S
    DevBuf<float> att_S; int att_split_pos = 0;
    bool split_merged = false;                             // the split form's scores ride in the qkv launch (launch_qkv_scores): one GPU, quantised files, LMRS_ATT_SPLIT_MERGED
    // batched forward_layer (fill_kv_cache): device buffers for kPrefillTokens tokens, allocated on first use
    DevBuf<float> pf_x, pf_q, pf_k, pf_ao, pf_h, pf_xs, pf_t; DevBuf<int8_t> pf_xq; DevBuf<float> pf_att;     // (pf_att: grown to a pass's score slabs, count() floats)
    bool pf_ready = false;                                 // every prefill buffer above is allocated
    // batched prefill on row shards (plan "tp", Q8_0): the gathered blocks of a token batch - per shard [n_tok x slice int8 | n_tok x slice / 128 scales],
    // pfb_att / pfb_h bytes apart; inside the peer-to-peer arena when that is the transport (peers write them), ordinary memory for RCCL
    char *pfx_att = nullptr, *pfx_h = nullptr, *pfx_x = nullptr; size_t pfb_att = 0, pfb_h = 0, pfb_x = 0; bool pfx_owned = false;   // pfx_x: the split-out plan's f32 slices of wo / w2's output
    bool tp_prefill = false;                               // decided at create (prefill_tp_shapes_ok: shapes and LMRS_NO_BATCHED_PREFILL) - where the blocks live follows from it
    float* x2 = nullptr; bool gemma_fused = false;           // Gemma: second residual buffer; norm+add steps folded into the consuming GEMV prologues
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    Switches sw;                                   // the environment switches, read at create (lmrs_switches.h)
    std::vector<DevBuf<float>> scales_t;           // the layers' transposed scale copies
    int att_dim = 0, kv_dim = 0, cls_grid = 0;     // att_dim / kv_dim: THIS shard's query / key-value widths
    int part_stride = 0;                           // floats between two shards' argmax partials: 2 * cls_grid rounded up to 16 bytes (the push transport copies 16 bytes per lane;
                                                   // Llama-3.2-1B on 8 shards has 501 partials per shard)
    bool q4 = false, f32 = false;                  // f32: q_type None (unquantised weights, lmrs_f32.inc)
    // ---- row sharding.  Every shard owns whole output rows, so every float accumulation chain
    // lives on one GPU and results are bit-identical to world == 1.
    int rank = 0, world = 1;
    int att_full = 0;                              // n_heads * head_size of the whole model
    int dim_l = 0, hid_l = 0, voc_l = 0;           // rows of wo/w2, gate-up pairs of w13, classifier rows owned here
    int d0 = 0, h0 = 0, v0 = 0, a0 = 0;            // first owned row / pair / vocab row / att column
    bool rep_out = true;                           // wo / w2 replicated (all dim rows on every shard): no gather after them
    bool cls_only = false;                         // shard plan "cls": the layers run whole on every shard, only the classifier's rows are split
    ncclComm_t comm = nullptr;                     // RCCL communicator (one process per GPU); null in group mode
    bool eager = false;                            // sharded step could not be captured: enqueue it every call
    float* part = nullptr;                         // [world][values(cls_grid) | indices(cls_grid)] argmax partials
    // quantised exchange payloads (Q8_0): one block per shard, [slice int8 | slice/128 f32 scales], blk_* bytes apart
    bool qpay = false; char *gq_att = nullptr, *gq_h = nullptr; size_t blk_att = 0, blk_h = 0;
    // peer-to-peer transport: every exchange buffer lives in one fine-grained allocation with the same layout on every shard;
    // a shard pushes its block straight into its peers' copies (xGMI stores) and raises a flag there (exchange_push_kernel)
    bool p2p = false, p2p_ready = false; char* xarena = nullptr; size_t xarena_bytes = 0; char* peer_base[kMaxWorld] = {};
    unsigned *xflags = nullptr, *xseq = nullptr; int* xerr = nullptr; int ex_slot = 0; bool xarena_is_ipc[kMaxWorld] = {};
    double last_fill_ms = -1.0;                    // device time of the last batched fill_kv_cache between its upload and its download (lmrs_last_fill_ms)
    bool err_queued = false;                       // the error word's copy to h_err rides in front of the call's own synchronise (queue_err)
    int* err = nullptr; PinBuf<int> h_err;         // error word of the bounded in-launch waits (merged qkv + attention launch, classifier tail)
    // ---- merged qkv + attention launch (launch_qkv_attn): per-layer {value, tag} granules, the step sequence number the tags are
    // made of (bumped by the last kernel of every step, never reset), and the graph of the separate kernels for the steps it does not cover
    // what enqueue_layer launches is StepForm::qa_mode: 0 the separate kernels, 1 merged with one workgroup per head (pos < qa_max_T), 2 merged with
    // one wave per head - per 64 keys of a 64-wide head - (pos < qa_wave_T)
    bool qkv_att = false; unsigned long long* gran = nullptr; unsigned* seq = nullptr; int qa_max_T = 0, qa_wave_T = 0;
    // several decode steps per graph launch (position and tokens live on the device, a step needs nothing from the host): lmrs_generate_greedy
    // replays the multi_k-step graph of a form while multi_k steps remain inside it
    int multi_k = 1;
    // ---- final argmax folded into the classifier launch (ClsTail): packed partials
    bool cls_tail = false; unsigned long long* part_pk = nullptr; unsigned* cls_seq = nullptr;
    int inj_fail_connect = 0, inj_stall_seg = -1; long long inj_stall_ticks = 0;      // lmrs_debug_inject
    // lmrs_forward_tokens / lmrs_score_tokens (allocated on first use): the [sc_rows][vocab] logits block, the reduction's chunk summaries,
    // its per-position results on the device and their pinned host copy
    DevBuf<float> sc_logits; int sc_rows = 0; DevBuf<ScorePart> sc_part; DevBuf<double> sc_lp; DevBuf<uint32_t> sc_idx; PinBuf<char> h_sc;
    // lmrs_score_tokens_topk / lmrs_forward_topk (allocated on first use, for tk_rows rows of tk_k candidates): the selection's keys and counts between
    // its two launches, the seq_len x tk_k results (index, value) and the seq_len target ranks, and their pinned host copy
    DevBuf<unsigned long long> tk_cand; DevBuf<uint32_t> tk_cnt, tk_idx; DevBuf<float> tk_val; DevBuf<uint32_t> tk_rank;
    PinBuf<char> h_tk; int tk_rows = 0, tk_k = 0;            // (tk_rows != 0: the set stands - alloc_all)

    template <class T> T* alloc(size_t count) {
        size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
        if (arena_used + bytes > arena_bytes) return nullptr;
        T* p = reinterpret_cast<T*>(arena + arena_used); arena_used += bytes; return p;
    }
};

namespace {

__global__ void advance_pos_kernel(DevState* st, unsigned* seq) { st->pos += 1; st->step_count += 1; *seq += 1u; }
__global__ void stall_kernel(long long ticks) { const long long t0 = wall_clock64(); while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32); }   // lmrs_debug_inject

size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

constexpr int kPrefillTokens = 512;            // tokens per pass of the batched forward_layer (fill_kv_cache, the prompt of generate_greedy)
// Batched prefill on ROW SHARDS (plan "tp"): the configurations it is built for - Q8_0 and Q4_0 with whole 128-groups of att_out / h per shard
// (a shard quantises ITS slice of every token's vector: bit for bit the groups of the gathered vector), wo / w2 replicated or split too (the
// split-out plan: two more all-gathers per layer, of f32 row slices), Llama / Phi head sizes and Gemma-2 (round 6: Q4_0, Gemma-2 and the split-out
// plan too); everything else feeds its tokens one by one.
bool prefill_tp_shapes_ok(const lmrs_ctx* c) {
    const lmrs_args& a = c->args;
    if (c->world < 1 || c->cls_only || c->f32 || c->sw.no_batched_prefill) return false;
    if (!c->rep_out && c->dim_l % 16) return false;                      // (the split-out plan: wo / w2 rows split too - their slices are whole GEMM row tiles' worth)
    if (a.q_type != LMRS_Q8_0 && a.q_type != LMRS_Q4_0) return false;
    if (c->att_dim % 128 || c->hid_l % 128) return false;
    if (!rows_prologue_supported((int)a.dim)) return false;
    if (a.model_type == LMRS_GEMMA) { if (a.head_size != 256 || a.dim != 2304) return false; }
    else if (a.head_size != 64 && a.head_size != 96 && a.head_size != 128) return false;
    return (c->att_dim + 2 * c->kv_dim) % 16 == 0 && c->kv_dim % 4 == 0 && a.dim % 16 == 0 && c->att_full % 128 == 0 && a.hidden_dim % 128 == 0;
}
// bytes of one shard's block for a slice of n_l values per token: [kPrefillTokens x n_l int8 | kPrefillTokens x n_l / 128 f32]
size_t prefill_tp_block(size_t n_l) { return pad256((size_t)kPrefillTokens * n_l + (size_t)kPrefillTokens * (n_l / 128) * 4); }

// The form of one decode step: how it runs qkv + attention (qa_mode, see lmrs_ctx::qkv_att) and, when its attention is the split pair, over how many
// 256-key chunks (then qa_mode is 0) - as the plain qkv launch, the score launch and the value launch, or, split_merged, with the scores inside the
// qkv launch (launch_qkv_scores).  A value handed down to the enqueue functions, never context state.
struct StepForm { int qa_mode = 0, split_chunks = 0; bool split_merged = false; };
// The form of one batched pass, a value in the same way: skinny = every GEMM of it, the layers' and the classifier's, in the weight-streaming forms (GemmArgs::skinny: up to 16 rows, a batch pass up to 64)
// rows: the pass is lmrs_batch_forward's - row r is one token of its own sequence (the device row table, lmrs_kernels.h; max_T = the deepest row's
// position + 1); null: m consecutive positions of one sequence, as always.  k_cache / v_cache: the caches the pass reads and writes - a batch's (with
// rows: the base the table's offsets count from); null: the context's own
// runs (runs.tok != null): the pass is lmrs_batch_forward_runs' - a table of up to kRunRowsMax rows, several of them consecutive positions of one slot; its
// qkv block is wider than pf_q at that many rows, so the pass brings a buffer of its own (qkv; null: pf_q, as every other pass).
// masks (masks.bits != null): some output row of the pass belongs to a batch slot with an allowed-token mask (lmrs_batch_set_masks) - of[r] is the mask row of
// output row r in the order the classifier sees the rows, -1 for none; h_of is its pinned source, which says on the host whether a slab has a masked row at all.
struct MaskView { const uint32_t* bits = nullptr; int words = 0; const int* of = nullptr; const int* h_of = nullptr; };
// autos (autos.of != null): some output row of the pass belongs to a slot with a token automaton (lmrs_batch_attach_automaton) - of[r] carries the automaton's
// tables and the slot, whose state word (state[slot]) the launch reads on the device; h_of is its pinned source, as with the masks
struct AutoView { const AutoRow* of = nullptr; const AutoRow* h_of = nullptr; const uint32_t* state = nullptr; int words = 0; };
// penalties (penalties.hist != null): some output row of the pass belongs to a slot with penalties (lmrs_batch_set_penalties) - of[r] carries slot, parameters and the
// table row whose position is row r's (pos: that column of the pass's device table, read on the device - right inside lmrs_batch_generate_greedy's loops); h_of is
// its pinned source, as with the masks; max_n = the deepest row's position + 1 at this pass (the keys a workgroup sorts)
// filters (filters.of != null): some output row of the pass belongs to a slot with candidate filters (lmrs_batch_set_filters) - of[r] carries the slot and its
// top_k / min_gap in the order the classifier sees the rows, slot -1 for none; h_of is its pinned source, as with the masks
struct FilterView { const FilterRow* of = nullptr; const FilterRow* h_of = nullptr; };
struct PenaltyView { const uint32_t* hist = nullptr; int seq_len = 0; const int* pos = nullptr; const PenaltyRow* of = nullptr; const PenaltyRow* h_of = nullptr; int max_n = 0; };
struct PassForm { bool skinny = false; const RowTable* rows = nullptr; int max_T = 0; float *k_cache = nullptr, *v_cache = nullptr; RowView runs{}; float* qkv = nullptr; PageView pages{}; MaskView masks{}; AutoView autos{}; PenaltyView penalties{}; FilterView filters{}; int block_pos0 = -1; uint32_t block_row = 0; };   // pages.tab != null: the table pass of a paged batch - k_cache / v_cache are the pool's, the rows' off words table rows; block_pos0 >= 0: its rows are the consecutive positions of ONE slot (page row block_row) from there on, in position order - block attention over the pages
// The whole rule, by position: split attention from att_split_pos on, bucket b covering positions below 1024 << b; below it the merged launch where
// it reaches.  merged = false: the separate kernels whatever the position (steps enqueued because the runtime refused to capture them, the layer
// passes of fill_kv_cache).
StepForm step_form_for(const lmrs_ctx* c, uint32_t pos, bool merged = true) {
    StepForm f;
    if (c->att_split_pos > 0 && (int)pos >= c->att_split_pos) {
        int b = 0;
        while (b < 3 && pos >= (1024u << b)) ++b;
        f.split_chunks = 4 << b;
        f.split_merged = merged && c->split_merged;
    } else if (merged && c->qkv_att) f.qa_mode = (int)pos < c->qa_wave_T ? 2 : ((int)pos < c->qa_max_T ? 1 : 0);
    return f;
}
// the score scratch of the split attention, allocated when the first split step is about to be enqueued
int split_scratch(lmrs_ctx* c, StepForm f) {
    if (!f.split_chunks || c->att_S) return 0;
    return c->att_S.alloc(attention_split_scratch_floats(c->att_dim / (int)c->args.head_size, (int)c->args.seq_len)) ? 0 : alloc_failed("split attention scores: hipMalloc");
}

// RoPE terms, transformer.rs:446-482 (libm powf/cosf/sinf/logf exactly where the reference calls them).
void rope_terms(const lmrs_args& a, uint32_t p, uint32_t j, float* fcr, float* fci) {
    static const double short_factor[48] = {   // transformer.rs:473
        1.08, 1.1, 1.1300000000000001, 1.2800000000000002, 1.3100000000000003, 1.4500000000000004, 1.4500000000000004,
        1.9500000000000008, 2.030000000000001, 2.4299999999999926, 2.5699999999999896, 2.9499999999999815, 3.729999999999965,
        3.869999999999962, 4.189999999999955, 4.43999999999995, 4.6399999999999455, 4.979999999999938, 5.159999999999934,
        5.279999999999932, 5.759999999999922, 5.889999999999919, 5.889999999999919, 5.969999999999917, 6.089999999999915,
        6.2799999999999105, 6.7699999999999, 6.8899999999998975, 7.109999999999893, 7.129999999999892, 7.179999999999891,
        7.289999999999889, 7.339999999999888, 7.559999999999883, 7.619999999999882, 7.69999999999988, 7.879999999999876,
        7.879999999999876, 7.879999999999876, 7.939999999999875, 7.949999999999875, 7.979999999999874, 8.19999999999987,
        8.439999999999864, 8.469999999999864, 8.589999999999861, 8.809999999999857, 8.999999999999853};
    const uint32_t head_dim = j * 2;
    float freq = 1.0f / powf(a.rope_theta, (float)head_dim / (float)a.head_size);
    float scaling_factor = 1.0f;
    if (a.model_type == LMRS_LLAMA) {                          // hard-coded Llama-3 scaling
        const float wavelen = (2.0f * 3.14159265358979323846f) / freq;
        const float factor = 32.0f, low_freq_factor = 1.0f, high_freq_factor = 4.0f, old_context_len = 8192.0f;
        const float low_freq_wavelen = old_context_len / low_freq_factor;
        const float high_freq_wavelen = old_context_len / high_freq_factor;
        if (wavelen > low_freq_wavelen) freq = freq / factor;
        else if (wavelen <= low_freq_wavelen && wavelen >= high_freq_wavelen) {
            const float smooth_factor = (old_context_len / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor);
            freq = (1.0f - smooth_factor) * freq / factor + smooth_factor * freq;
        }
    }
    if (a.model_type == LMRS_PHI) {                            // LongRoPE short factors + long magnitude
        freq = freq * (float)(1.0 / short_factor[j]);          // j < 48: checked at create
        const float scale = 131072.0f / 4096.0f;
        scaling_factor = sqrtf(1.0f + logf(scale) / logf(4096.0f));
    }
    const float val = (float)p * freq;
    *fcr = cosf(val) * scaling_factor;
    *fci = sinf(val) * scaling_factor;
}

extern "C" int lmrs_rope_terms(const lmrs_args* args, uint32_t pos, uint32_t j, float* fcr, float* fci) {
    if (!args || !fcr || !fci) return fail("NULL argument");
    if (args->head_size < 2 || j >= args->head_size / 2) return fail("j must be below head_size / 2");
    if (args->model_type == LMRS_PHI && args->head_size > 96) return fail("Phi: head_size above 96 indexes past the 48 LongRoPE short factors");
    rope_terms(*args, pos, j, fcr, fci);
    return 0;
}

// one decoder layer of an unquantised model (q_type None): the same launches with the f32 matmul (lmrs_f32.inc); Gemma's
// x += rmsnorm(branch) steps as separate launches
int enqueue_layer_f32(lmrs_ctx* c, StepForm f, int l) {
    const lmrs_args& a = c->args;
    const DevLayer& L = c->layers[l];
    const bool gemma = a.model_type == LMRS_GEMMA;
    GemvArgs g{};
    g.eps = a.rms_norm_eps; g.add_unit = gemma; g.st = c->st;
    g.att_dim = c->att_dim; g.kv_dim = c->kv_dim; g.seq_len = a.seq_len; g.layer = l;
    set_launch_tag(0);
    g.wq = L.wqkv; g.n = a.dim; g.o = c->att_dim + 2 * c->kv_dim; g.xin = c->x; g.rms_w = L.rms_att; g.out = c->q; g.k_raw = c->k_raw; g.v_cache = c->v_cache;
    HIP_OK(launch_gemv_f32(g, PRO_RMS_QUANT, EPI_QKV, c->stream));
    AttnArgs t{};
    t.q = c->q; t.k_raw = c->k_raw; t.k_cache = c->k_cache; t.v_cache = c->v_cache; t.rope = c->rope; t.out = c->att_out;
    t.n_heads = a.n_heads; t.n_kv_heads = a.n_kv_heads; t.head_size = a.head_size; t.seq_len = a.seq_len; t.layer = l; t.gemma = gemma; t.st = c->st;
    set_launch_tag(1);
    if (f.split_chunks) HIP_OK(launch_attention_split(t, c->att_S, f.split_chunks, c->stream));
    else HIP_OK(launch_attention(t, c->stream));
    set_launch_tag(2);
    g.wq = L.wo; g.n = c->att_dim; g.o = a.dim; g.xin = c->att_out; g.out = gemma ? c->tmp : c->x;
    HIP_OK(launch_gemv_f32(g, PRO_QUANT, gemma ? EPI_STORE : EPI_RESID, c->stream));
    set_launch_tag(7);
    if (gemma) HIP_OK(launch_addnorm(c->x, c->tmp, L.rms_post_att, a.dim, a.rms_norm_eps, c->stream));
    set_launch_tag(3);
    g.wq = L.w13; g.n = a.dim; g.o = 2 * a.hidden_dim; g.xin = c->x; g.rms_w = gemma ? L.rms_pre_ffn : L.rms_post_att; g.out = c->h;
    HIP_OK(launch_gemv_f32(g, PRO_RMS_QUANT, gemma ? EPI_GELU : EPI_SWIGLU, c->stream));
    set_launch_tag(4);
    g.wq = L.w2; g.n = a.hidden_dim; g.o = a.dim; g.xin = c->h; g.out = gemma ? c->tmp : c->x;
    HIP_OK(launch_gemv_f32(g, PRO_QUANT, gemma ? EPI_STORE : EPI_RESID, c->stream));
    set_launch_tag(7);
    if (gemma) HIP_OK(launch_addnorm(c->x, c->tmp, L.rms_post_ffn, a.dim, a.rms_norm_eps, c->stream));
    return 0;
}

// one decoder layer (transformer.rs:388-657) as 5 fused launches
int enqueue_layer(lmrs_ctx* c, StepForm f, int l) {
    if (c->f32) return enqueue_layer_f32(c, f, l);
    const lmrs_args& a = c->args;
    const DevLayer& L = c->layers[l];
    const bool gemma = a.model_type == LMRS_GEMMA;
    GemvArgs g{};
    g.q4 = c->q4; g.eps = a.rms_norm_eps; g.add_unit = gemma; g.st = c->st;
    g.att_dim = c->att_dim; g.kv_dim = c->kv_dim; g.seq_len = a.seq_len; g.layer = l;
    // 1. rmsnorm + quantize | Wqkv | q, raw k, v -> cache            (:409-431)
    g.wq = L.wqkv; g.ws = L.sqkv; g.n = a.dim; g.o = c->att_dim + 2 * c->kv_dim;
    g.xin = c->x; g.rms_w = L.rms_att; g.out = c->q; g.k_raw = c->k_raw; g.v_cache = c->v_cache;
    g.att_dim = c->att_dim; g.kv_dim = c->kv_dim; g.seq_len = a.seq_len; g.layer = l;
    g.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    set_launch_tag(0);
    // Gemma, folded form: the residual lives in x at the top of a layer except that, from layer 1 on, the previous
    // layer's "x += rmsnorm(ffn_out, post_ffn)" (:643-650) is still pending in (x2, tmp): this prologue applies it, x2 -> x.
    const bool pending = c->gemma_fused && l > 0;
    if (pending) { g.xin = c->x2; g.delta = c->tmp; g.add_w = c->layers[l - 1].rms_post_ffn; g.xout = c->x; }
    AttnArgs t{};
    t.q = c->q; t.k_raw = c->k_raw; t.k_cache = c->k_cache; t.v_cache = c->v_cache; t.rope = c->rope; t.out = c->att_out;
    t.n_heads = a.n_heads; t.n_kv_heads = a.n_kv_heads; t.head_size = a.head_size; t.seq_len = a.seq_len; t.layer = l;
    t.gemma = gemma; t.st = c->st;
    if (f.split_chunks && f.split_merged) {
        // 1 + the scores of 2 as ONE launch: the (head, key chunk) score items poll the granules the qkv workgroups write (launch_qkv_scores); then the values
        g.gran = c->gran + (size_t)l * (c->att_dim + 2 * c->kv_dim); g.seq = c->seq;
        HIP_OK(launch_qkv_scores(g, pending ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, t, c->att_S, c->err, f.split_chunks, c->sw.att_split_score_wgs, c->stream));
        g.gran = nullptr; g.seq = nullptr;
        t.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
        set_launch_tag(1);
        HIP_OK(launch_attention_split_values(t, c->att_S, c->stream));
    } else if (f.qa_mode && !f.split_chunks) {
        // 1 + 2 as ONE launch: the attention workgroups poll the granules the qkv workgroups write (launch_qkv_attn)
        g.gran = c->gran + (size_t)l * (c->att_dim + 2 * c->kv_dim); g.seq = c->seq;
        t.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
        HIP_OK(launch_qkv_attn(g, pending ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, t, c->err, c->qa_max_T, f.qa_mode == 2, c->stream));
        g.gran = nullptr; g.seq = nullptr;
    } else {
    HIP_OK(launch_gemv(g, pending ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, EPI_QKV, c->stream));
    // 2. RoPE + attention                                               (:443-544)
    t.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    set_launch_tag(1);
    if (f.split_chunks) HIP_OK(launch_attention_split(t, c->att_S, f.split_chunks, c->stream));
    else HIP_OK(launch_attention(t, c->stream));
    }
    g.delta = nullptr; g.add_w = nullptr; g.xout = nullptr;
    // 3. quantize | Wo | x += ...                                       (:550-576)
    g.wq = L.wo; g.ws = L.so; g.n = c->att_dim; g.o = a.dim; g.xin = c->att_out; g.out = gemma ? c->tmp : c->x;
    g.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    set_launch_tag(2);
    HIP_OK(launch_gemv(g, PRO_QUANT, gemma ? EPI_STORE : EPI_RESID, c->stream));
    set_launch_tag(7);
    if (gemma && !c->gemma_fused) HIP_OK(launch_addnorm(c->x, c->tmp, L.rms_post_att, a.dim, a.rms_norm_eps, c->stream));   // :563-568
    // 4. rmsnorm + quantize | W1,W3 interleaved | silu(g)*u             (:578-624)
    g.wq = L.w13; g.ws = L.s13; g.n = a.dim; g.o = 2 * a.hidden_dim; g.xin = c->x; g.rms_w = gemma ? L.rms_pre_ffn : L.rms_post_att; g.out = c->h;
    g.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    if (c->gemma_fused) { g.delta = c->tmp; g.add_w = L.rms_post_att; g.xout = c->x2; }      // x2 = x + rmsnorm(wo_out, post_att) (:563-568), then pre_ffn norm
    set_launch_tag(3);
    HIP_OK(launch_gemv(g, c->gemma_fused ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, gemma ? EPI_GELU : EPI_SWIGLU, c->stream));
    g.delta = nullptr; g.add_w = nullptr; g.xout = nullptr;
    // 5. quantize | W2 | x += ...                                       (:630-654)
    g.wq = L.w2; g.ws = L.s2; g.n = a.hidden_dim; g.o = a.dim; g.xin = c->h; g.out = gemma ? c->tmp : c->x;
    g.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    set_launch_tag(4);
    HIP_OK(launch_gemv(g, PRO_QUANT, gemma ? EPI_STORE : EPI_RESID, c->stream));
    set_launch_tag(7);
    if (gemma && !c->gemma_fused) HIP_OK(launch_addnorm(c->x, c->tmp, L.rms_post_ffn, a.dim, a.rms_norm_eps, c->stream));   // :643-650
    return 0;
}

// Folded Gemma form: after the last layer "x2 += rmsnorm(tmp, post_ffn)" is still pending (the classifier's prologue
// applies it); callers that need the finished residual stream in x (fill_kv_cache) run this instead.
int enqueue_finish_residual(lmrs_ctx* c) {
    if (!c->gemma_fused) return 0;
    const lmrs_args& a = c->args;
    HIP_OK(launch_addnorm(c->x2, c->tmp, c->layers[a.n_layers - 1].rms_post_ffn, a.dim, a.rms_norm_eps, c->stream));
    HIP_OK(hipMemcpyAsync(c->x, c->x2, (size_t)a.dim * 4, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

// classifier rows this context computes: its slice of the vocabulary, cut at the last multiple of 4 of the whole vocabulary
static int cls_rows(const lmrs_ctx* c) {
    if (c->q4) return c->voc_l;                          // matmul_q4 walks every row (par_iter_mut, functional.rs:226): no unwritten tail
    const int written = (int)(c->args.vocab_size & ~3u) - c->v0;
    return written < c->voc_l ? (written > 0 ? written : 0) : c->voc_l;
}

// first of the never-written logits (they hold 0.0), or 0 when the vocabulary is a multiple of 4
static int unwritten_tail(const lmrs_ctx* c) { return !c->q4 && c->args.vocab_size % 4 ? (int)(c->args.vocab_size & ~3u) : 0; }

GemvArgs cls_args(lmrs_ctx* c) {
    const lmrs_args& a = c->args;
    GemvArgs g{};
    g.q4 = c->q4; g.eps = a.rms_norm_eps; g.add_unit = a.model_type == LMRS_GEMMA; g.st = c->st;
    const size_t row_bytes = c->f32 ? (size_t)a.dim * 4 : (c->q4 ? a.dim / 2 : a.dim);
    g.wq = static_cast<const char*>(c->cls_q) + (size_t)c->v0 * row_bytes; g.ws = c->f32 ? nullptr : c->cls_s + (size_t)c->v0 * (a.dim / 128);
    // matmul_q8 / matmul (not matmul_q4) hand out the output rows four at a time (par_chunks_exact_mut(4), functional.rs:148,179): the last
    // vocab_size % 4 logits are never written - they keep the 0.0 the buffer was created with, and argmax sees them as 0.0
    g.n = a.dim; g.o = cls_rows(c); g.xin = c->x; g.rms_w = c->rms_final; g.row_offset = c->v0;
    g.out = c->logits + c->v0;
    if (c->world > 1 || c->comm) {          // sharded: this shard's [values | indices] block of the gathered partials
        g.part_val = c->part + (size_t)c->rank * c->part_stride;
        g.part_idx = reinterpret_cast<int*>(c->part + (size_t)c->rank * c->part_stride) + c->cls_grid;
        if (c->p2p) { g.part_par = c->xseq + c->ex_slot; g.part_par_floats = (int)((size_t)c->world * 2 * kMaxArgmaxParts); }   // the exchange enqueued next takes this slot
    } else { g.part_val = c->part_val; g.part_idx = c->part_idx; }
    g.softcap_rows = a.model_type == LMRS_GEMMA ? (int)a.dim : 0;
    if (c->gemma_fused) { g.xin = c->x2; g.delta = c->tmp; g.add_w = c->layers[a.n_layers - 1].rms_post_ffn; g.xout = c->x; }
    return g;
}

EmbedArgs embed_args(lmrs_ctx* c) {
    const lmrs_args& a = c->args;
    EmbedArgs e{};
    e.emb_q = c->emb_q; e.emb_s = c->emb_s; e.q4 = c->f32 ? 2 : (int)c->q4; e.tokens = c->tokens; e.x = c->x; e.dim = a.dim;
    e.do_scale = a.model_type == LMRS_GEMMA; e.scale = sqrtf((float)a.dim); e.st = c->st;
    return e;
}

// One decode step minus the embedding of its input token: that row is produced by the previous step's
// argmax kernel (or by launch_embed for the first step of a call), which saves a dependent launch per token.
int enqueue_step(lmrs_ctx* c, StepForm f) {
    const lmrs_args& a = c->args;
    for (uint32_t l = 0; l < a.n_layers; ++l) if (enqueue_layer(c, f, (int)l)) return -1;
    GemvArgs g = cls_args(c);                                   // final rmsnorm + quantize | classifier | argmax partials (:341-381)
    g.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    set_launch_tag(5);
    ArgmaxArgs m{};
    m.part_val = c->part_val; m.part_idx = c->part_idx; m.n_part = c->cls_grid; m.n_groups = 1; m.group_stride = 0; m.logits = c->logits; m.tail_row = unwritten_tail(c); m.tokens = c->tokens; m.st = c->st; m.seq = c->seq; m.emb = embed_args(c);
    if (c->cls_tail) {                                          // one GPU: the classifier's last-arriving workgroup finishes the step itself
        g.has_tail = 1; g.tail.part_pk = c->part_pk; g.tail.err = c->err; g.tail.cls_seq = c->cls_seq; g.tail.m = m;
        HIP_OK(launch_gemv(g, c->gemma_fused ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, EPI_CLS, c->stream));
        return 0;
    }
    if (c->f32) HIP_OK(launch_gemv_f32(g, PRO_RMS_QUANT, EPI_CLS, c->stream));
    else HIP_OK(launch_gemv(g, c->gemma_fused ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, EPI_CLS, c->stream));
    set_launch_tag(6);
    m.dbg = c->dbg ? c->dbg + 8 * (c->dbg_node++) : nullptr;
    HIP_OK(launch_argmax_final(m, c->stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Row-sharded step (world > 1), cut into segments at the points where every shard needs the others' rows.
//   segment 4l+0: [pending residual update] qkv(own heads) -> attention(own heads) [-> quantise own att_out slice]   exchange att
//   segment 4l+1: wo (all rows if replicated, else own rows)                                                          [exchange tmp]
//   segment 4l+2: [residual update] w1/w3 (own pairs) -> act(gate)*up [-> quantise own h slice]                        exchange h
//   segment 4l+3: w2 (all rows if replicated, else own rows)                                                          [exchange tmp]
//   segment 4L  : [residual update] classifier (own vocab rows) + argmax partials                                      exchange partials
//   segment 4L+1: argmax over all shards' partials, next-token embedding (replicated)
// Residual update: Llama / Phi add the projection's output (in the GEMV epilogue when wo / w2 are replicated, else x += tmp after
// the exchange); Gemma-2 always goes through tmp: x += rmsnorm(tmp, post_att / post_ffn) (transformer.rs:563-568, 643-650).
// Exchanges are in place: shard r's block sits at buf + r * stride on every shard.  Payloads:
//   * Q8_0 models: att_out and h travel QUANTISED - the producing shard runs the reference's quantize (quantization.rs:44-67) on
//     its own slice (whole 128-groups: bit-identical to quantising the gathered vector) and ships int8 + one f32 scale per group,
//     3.9x fewer bytes than f32, and the consumers (wo, w2) start from the quantised vector (PRO_PREQ, sliced) instead of each of
//     their workgroups re-quantising it.  Q4_0 models and LMRS_SHARD_F32_PAYLOAD=1: f32 slices.
//   * tmp slices (fully row-split form) and the argmax partials: f32 / raw.
// ------------------------------------------------------------------------------------------------
struct ExchangeDesc { char* buf; size_t bytes, stride; const float* qsrc; size_t qn; size_t par = 0; bool wide = false; };   // wide: a token batch's block (copied by many workgroups)   // par > 0: double-buffered block, halves `par` bytes apart (exchange_push_kernel picks the half by its sequence number)   // bytes valid per shard, blocks `stride` bytes apart (in place); qsrc: f32 slice still to be quantised into this shard's block
// Which matrices to split over `world` GPUs.  Row-splitting a layer's matrices costs two exchanges per layer (four in the fully split
// form): pure latency, a few microseconds each, every layer of every token.  It pays only when the gate / up / down stream a shard no
// longer reads is longer than that: (w1 + w3 + w2 bytes per layer) x (1 - 1/world) at the ~6.3 TB/s a GPU streams, against ~9 us for two
// exchanges - about 57 MB.  Below that (the 1B and 2B models at any world size, the 3B / 3.8B ones at 2 and 4) the plan is "cls": every shard
// runs the layers whole, with the fused single-GPU kernels and no exchange, and only the classifier - the one big stream of the step,
// 270 MB for Llama-3.2 - is row-split, for ONE exchange of the argmax partials per token.  LMRS_SHARD_PLAN=tp|cls overrides.
static bool shard_plan_cls_only(const lmrs_args& a, int world, const Switches& sw) {
    if (world <= 1) return false;
    if (sw.shard_plan) return sw.shard_plan == 1;
    const double bpe = a.q_type == LMRS_Q4_0 ? 0.5 + 4.0 / 128 : 1.0 + 4.0 / 128;
    const double mlp_bytes = 3.0 * a.dim * a.hidden_dim * bpe;
    return mlp_bytes * (1.0 - 1.0 / world) < 57e6;
}

int n_segments(const lmrs_ctx* c) { return 4 * (int)c->args.n_layers + 2; }

static size_t part_half_floats(const lmrs_ctx* c) { return (size_t)c->world * 2 * kMaxArgmaxParts; }
ExchangeDesc exchange_after(lmrs_ctx* c, int seg) {
    const int L4 = 4 * (int)c->args.n_layers;
    const ExchangeDesc none{nullptr, 0, 0, nullptr, 0};
    auto f32s = [](float* p, size_t count) { return ExchangeDesc{reinterpret_cast<char*>(p), count * 4, count * 4, nullptr, 0}; };
    if (c->cls_only && seg < L4) return none;                     // plan "cls": nothing is exchanged inside the layers
    if (seg < L4) {
        switch (seg & 3) {
            case 0: return c->qpay ? ExchangeDesc{c->gq_att, (size_t)c->att_dim + (size_t)c->att_dim / 32, c->blk_att, c->p2p ? c->att_out + c->a0 : nullptr, (size_t)c->att_dim} : f32s(c->att_out, (size_t)c->att_dim);
            case 2: return c->qpay ? ExchangeDesc{c->gq_h, (size_t)c->hid_l + (size_t)c->hid_l / 32, c->blk_h, c->p2p ? c->h + c->h0 : nullptr, (size_t)c->hid_l} : f32s(c->h, (size_t)c->hid_l);
            default: return c->rep_out ? none : f32s(c->tmp, (size_t)c->dim_l);
        }
    }
    if (seg == L4) {                                             // peer-to-peer: the partials are double-buffered (ArgmaxArgs::part_par)
        ExchangeDesc e = f32s(c->part, (size_t)c->part_stride);
        if (c->p2p) e.par = part_half_floats(c) * 4;
        return e;
    }
    return none;
}

// layers_only: the per-layer segments without classifier / argmax (fill_kv_cache on a sharded context: the finished residual in x)
int run_segment(lmrs_ctx* c, StepForm f, int seg) {
    const lmrs_args& a = c->args;
    const int L4 = 4 * (int)a.n_layers;
    // plan "cls": a layer is the five fused launches of the single-GPU step (its first segment runs all of it)
    if (c->cls_only && seg < L4) return (seg & 3) == 0 ? enqueue_layer(c, f, seg >> 2) : 0;
    const bool gemma = a.model_type == LMRS_GEMMA;
    GemvArgs g{};
    g.q4 = c->q4; g.eps = a.rms_norm_eps; g.add_unit = gemma; g.st = c->st;
    // the residual update that the PREVIOUS projection left pending
    auto pending_update = [&](const float* norm_w) -> int {
        set_launch_tag(7);
        if (gemma) HIP_OK(launch_addnorm(c->x, c->tmp, norm_w, a.dim, a.rms_norm_eps, c->stream));       // x += rmsnorm(tmp, 1 + w)
        else if (!c->rep_out) HIP_OK(launch_addvec(c->x, c->tmp, a.dim, c->stream));                      // x += tmp
        return 0;
    };
    // wo / w2: input quantised by its producers (sliced PRO_PREQ) or f32 (PRO_QUANT); output into x (+=) or tmp
    auto projection = [&](const void* wq, const float* ws, int n, const float* xin, const char* gq, int slice, size_t blk) -> int {
        g.wq = wq; g.ws = ws; g.n = n; g.o = c->dim_l;
        const bool to_tmp = gemma || !c->rep_out;
        g.out = to_tmp ? c->tmp + c->d0 : c->x;
        set_launch_tag(n == (int)a.hidden_dim ? 4 : 2);
        int pro = PRO_QUANT;
        if (c->qpay) { pro = PRO_PREQ; g.xq_in = gq; g.preq_slice = slice; g.preq_block = (int)blk; } else g.xin = xin;
        HIP_OK(launch_gemv(g, pro, to_tmp ? EPI_STORE : EPI_RESID, c->stream));
        return 0;
    };
    if (seg < L4) {
        const int l = seg >> 2; const DevLayer& L = c->layers[l];
        switch (seg & 3) {
            case 0: {
                if (l > 0 && pending_update(c->layers[l - 1].rms_post_ffn)) return -1;
                g.wq = L.wqkv; g.ws = L.sqkv; g.n = a.dim; g.o = c->att_dim + 2 * c->kv_dim;
                g.xin = c->x; g.rms_w = L.rms_att; g.out = c->q; g.k_raw = c->k_raw; g.v_cache = c->v_cache;
                g.att_dim = c->att_dim; g.kv_dim = c->kv_dim; g.seq_len = a.seq_len; g.layer = l;
                set_launch_tag(0);
                HIP_OK(launch_gemv(g, PRO_RMS_QUANT, EPI_QKV, c->stream));
                set_launch_tag(1);
                AttnArgs t{};
                t.q = c->q; t.k_raw = c->k_raw; t.k_cache = c->k_cache; t.v_cache = c->v_cache; t.rope = c->rope;
                t.out = c->att_out + c->a0;
                t.n_heads = c->att_dim / a.head_size; t.n_kv_heads = c->kv_dim / a.head_size; t.head_size = a.head_size;
                t.seq_len = a.seq_len; t.layer = l; t.gemma = gemma; t.st = c->st;
                if (f.split_chunks) HIP_OK(launch_attention_split(t, c->att_S, f.split_chunks, c->stream));
                else HIP_OK(launch_attention(t, c->stream));
                set_launch_tag(7);
                if (c->qpay && !c->p2p) {
                    char* blk = c->gq_att + (size_t)c->rank * c->blk_att;
                    HIP_OK(launch_quantize(c->att_out + c->a0, blk, reinterpret_cast<float*>(blk + c->att_dim), c->att_dim, 0, c->stream));
                }
                break;
            }
            case 1:
                if (projection(L.wo, L.so, c->att_full, c->att_out, c->gq_att, c->att_dim, c->blk_att)) return -1;
                break;
            case 2:
                if (pending_update(L.rms_post_att)) return -1;
                g.wq = L.w13; g.ws = L.s13; g.n = a.dim; g.o = 2 * c->hid_l; g.xin = c->x; g.rms_w = gemma ? L.rms_pre_ffn : L.rms_post_att; g.out = c->h + c->h0;
                set_launch_tag(3);
                HIP_OK(launch_gemv(g, PRO_RMS_QUANT, gemma ? EPI_GELU : EPI_SWIGLU, c->stream));
                set_launch_tag(7);
                if (c->qpay && !c->p2p) {
                    char* blk = c->gq_h + (size_t)c->rank * c->blk_h;
                    HIP_OK(launch_quantize(c->h + c->h0, blk, reinterpret_cast<float*>(blk + c->hid_l), c->hid_l, 0, c->stream));
                }
                break;
            default:
                if (projection(L.w2, L.s2, (int)a.hidden_dim, c->h, c->gq_h, c->hid_l, c->blk_h)) return -1;
                break;
        }
        return 0;
    }
    if (seg == L4) {
        if (!c->cls_only && pending_update(c->layers[a.n_layers - 1].rms_post_ffn)) return -1;      // ("cls": the layer finished its own residual)
        GemvArgs k = cls_args(c);
        set_launch_tag(5);
        HIP_OK(launch_gemv(k, PRO_RMS_QUANT, EPI_CLS, c->stream));
        return 0;
    }
    set_launch_tag(6);
    ArgmaxArgs m{};
    m.part_val = c->part; m.part_idx = reinterpret_cast<const int*>(c->part) + c->cls_grid; m.n_part = c->cls_grid;
    m.n_groups = c->world; m.group_stride = c->part_stride;
    if (c->p2p && c->ex_slot > 0) { m.part_par = c->xseq + (c->ex_slot - 1); m.part_par_floats = (int)part_half_floats(c); }     // the slot of the partials exchange just enqueued
    m.logits = c->logits; m.tokens = c->tokens; m.st = c->st; m.seq = c->seq; m.emb = embed_args(c); m.tail_row = unwritten_tail(c);
    HIP_OK(launch_argmax_final(m, c->stream));
    return 0;
}

#define NCCL_OK(expr)                                                                                    \
    do {                                                                                                 \
        ncclResult_t r_ = (expr);                                                                        \
        if (r_ != ncclSuccess) return fail(std::string(#expr) + ": " + ncclGetErrorString(r_));          \
    } while (0)

int enqueue_exchange(lmrs_ctx* c, const ExchangeDesc& e);     // P2P push kernel or RCCL all-gather (below)

// the sharded step (or only its layer segments) on this shard's stream, exchanges between the segments; every step takes the exchange slots from 0
int enqueue_step_sharded(lmrs_ctx* c, StepForm f, bool layers_only = false) {
    const int ns = layers_only ? 4 * (int)c->args.n_layers : n_segments(c);
    c->ex_slot = 0;
    for (int s = 0; s < ns; ++s) {
        if (run_segment(c, f, s)) return -1;
        const ExchangeDesc e = exchange_after(c, s);
        if (e.buf && enqueue_exchange(c, e)) return -1;
        if (e.buf && s == c->inj_stall_seg) hipLaunchKernelGGL(stall_kernel, dim3(1), dim3(1), 0, c->stream, c->inj_stall_ticks);
    }
    if (layers_only) {          // the last layer's residual update, so that x holds the finished residual stream; advance the position
        const lmrs_args& a = c->args;
        if (c->cls_only) {}                                        // (whole layers: x is already the finished residual)
        else if (a.model_type == LMRS_GEMMA) HIP_OK(launch_addnorm(c->x, c->tmp, c->layers[a.n_layers - 1].rms_post_ffn, a.dim, a.rms_norm_eps, c->stream));
        else if (!c->rep_out) HIP_OK(launch_addvec(c->x, c->tmp, a.dim, c->stream));
        hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, c->stream, c->st, c->seq);
    }
    return 0;
}

// ---- peer-to-peer exchange (the alternative to ncclAllGather for these latency-bound, few-KB messages) -------------------
// One workgroup: copy my block into the same place of every peer's exchange arena (stores that leave over xGMI; in the
// single-device verification modes the "peers" are other contexts / processes on the same GPU), make them visible system-wide,
// raise my flag in every peer's flag row with this exchange's sequence number, then wait until every peer's flag in MY row has
// reached it.  The arena is fine-grained (uncached in L2) memory, so the kernels that follow read what the peers wrote.
// Flags are monotonic per (exchange slot of the step, source shard): no reset, no ABA; all shards run the same sequence of steps.
constexpr int kMaxExchangeSlots = 512;

int enqueue_exchange(lmrs_ctx* c, const ExchangeDesc& e) {
    if (c->p2p) {
        if (!c->p2p_ready) return fail("peer-to-peer transport: peers not connected yet (lmrs_p2p_connect)");
        if (c->ex_slot >= kMaxExchangeSlots) return fail("too many exchanges in one step");
        if (e.stride % 16) return fail("peer-to-peer exchange: blocks must be 16-byte multiples");     // the push kernel copies 16 bytes per lane
        ExchangeArgs x{};
        const size_t off = (size_t)(e.buf - c->xarena) + (size_t)c->rank * e.stride;
        x.local = c->xarena + off; x.bytes = (int)((e.bytes + 15) & ~(size_t)15); x.rank = c->rank; x.world = c->world; x.slot = c->ex_slot;
        for (int w = 0; w < c->world; ++w) {
            x.peer_dst[w] = c->peer_base[w] + off;
            x.peer_flag[w] = reinterpret_cast<unsigned*>(c->peer_base[w] + ((char*)c->xflags - c->xarena)) + (size_t)c->ex_slot * kMaxWorld + c->rank;
        }
        x.my_flags = c->xflags + (size_t)c->ex_slot * kMaxWorld; x.my_seq = c->xseq + c->ex_slot; x.err = c->xerr;
        x.timeout_ticks = c->sw.p2p_timeout_ms * 100000ll;   // 100 MHz wall clock
        ++c->ex_slot;
        x.par_bytes = (int)e.par;
        if (e.qsrc) { x.qsrc = e.qsrc; x.qn = (int)e.qn; }      // the slice is quantised by the exchange kernel itself on its way out
        set_launch_tag(8);
        HIP_OK(e.wide ? launch_exchange_copy_push(x, c->stream) : launch_exchange_push(x, c->stream));
        return 0;
    }
    if (!c->comm) return fail("this context is a member of a lock-step shard group: drive it with lmrs_group_forward");
    NCCL_OK(ncclAllGather(e.buf + (size_t)c->rank * e.stride, e.buf, e.stride, ncclUint8, c->comm, c->stream));
    return 0;
}

int capture(lmrs_ctx* c, StepForm f, bool full, hipGraphExec_t* out, int n_steps = 1) {
    hipGraph_t graph = nullptr;
    c->dbg_node = 0;
    HIP_OK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = 0;
    if (full) { for (int k = 0; k < n_steps && !rc; ++k) rc = c->world > 1 || c->comm ? enqueue_step_sharded(c, f) : enqueue_step(c, f); }
    else {
        for (uint32_t l = 0; l < c->args.n_layers && !rc; ++l) rc = enqueue_layer(c, f, (int)l);
        if (!rc) rc = enqueue_finish_residual(c);
        if (!rc) hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(1), 0, c->stream, c->st, c->seq);
    }
    hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return -1; }
    if (e != hipSuccess) return fail(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    e = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    return 0;
}

// ---- the table of step graphs (lmrs_ctx::g_steps): the graph of `k` steps of form `f`, captured when it is not there yet; null: the capture failed
hipGraphExec_t step_graph(lmrs_ctx* c, StepForm f, int k = 1) {
    hipGraphExec_t& g = c->g_steps[f.split_chunks ? __builtin_ctz(f.split_chunks) + (f.split_merged ? 5 : 1) : f.qa_mode][k > 1];      // (chunks 4, 8, 16, 32 -> 3 .. 6, scores in the qkv launch: 7 .. 10)
    if (!g && capture(c, f, true, &g, k)) g = nullptr;
    return g;
}
int replay_steps(lmrs_ctx* c, StepForm f, int k = 1) {
    hipGraphExec_t g = step_graph(c, f, k);
    if (!g) return -1;
    HIP_OK(hipGraphLaunch(g, c->stream));
    return 0;
}
// the graph a context that replays graphs always has: one step of position 0's form (captured at create; sharded contexts: when the runtime accepted it)
hipGraphExec_t primary_graph(const lmrs_ctx* c) { return c->g_steps[step_form_for(c, 0).qa_mode][0]; }
// a sharded context's primary graph - or, when the runtime refuses the exchanges inside a capture, every step enqueued call by call
void capture_sharded_step(lmrs_ctx* c) {
    if (!step_graph(c, step_form_for(c, 0))) { c->eager = true; (void)hipGetLastError(); g_err.clear(); }
}
void destroy_step_graphs(lmrs_ctx* c) {
    for (auto& forms : c->g_steps) for (hipGraphExec_t& g : forms) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
}

// host->device copy of one tensor payload, optionally row-interleaved (dst row = 2*r + phase)
int upload(lmrs_ctx* c, void* dst, const uint8_t* src, size_t bytes) {
    HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}
int upload_interleaved(lmrs_ctx* c, void* dst, const uint8_t* src, size_t row_bytes, size_t rows, int phase) {
    HIP_OK(hipMemcpy2DAsync(static_cast<char*>(dst) + phase * row_bytes, 2 * row_bytes, src, row_bytes, row_bytes, rows,
                            hipMemcpyHostToDevice, c->stream));
    return 0;
}

// Every call gets its own pinned slot: the copy is asynchronous, so rewriting ONE slot twice inside an API call (the batched
// fill_kv_cache does) could overtake the first copy.  No API call issues more than a handful between two stream syncs.
constexpr unsigned kStateSlots = 16;
int set_state(lmrs_ctx* c, uint32_t pos, uint32_t prompt_end, int win_base = -1) {
    DevState* hs = c->h_st + (c->h_st_next++ % kStateSlots);
    hs->pos = (int)pos; hs->prompt_end = (int)prompt_end; hs->step_count = 0; hs->win_base = win_base;
    HIP_OK(hipMemcpyAsync(c->st, hs, sizeof(DevState), hipMemcpyHostToDevice, c->stream));
    if (c->qkv_att || c->cls_tail) HIP_OK(hipMemsetAsync(c->err, 0, 4, c->stream));   // (the three-part launch implies qkv_att)                // the error word of the bounded in-launch waits starts every call from zero
    return 0;
}

// after a host sync: did a bounded in-launch wait give up?
// the in-launch waits' error word -> pinned host memory, queued on the stream BEFORE the synchronise every call ends with: the check then
// costs no round trip of its own (a blocking 4-byte copy per token was ~10 us on a path trimmed by microseconds)
int queue_err(lmrs_ctx* c) {
    if (!c->err || !(c->qkv_att || c->cls_tail)) return 0;
    HIP_OK(hipMemcpyAsync(c->h_err, c->err, 4, hipMemcpyDeviceToHost, c->stream));
    c->err_queued = true;
    return 0;
}
int check_err(lmrs_ctx* c) {
    const bool queued = c->err_queued;                           // (cleared on EVERY path out of here: a stale flag would make a later call skip the copy)
    c->err_queued = false;
    if (c->xerr) {
        int e = 0;
        HIP_OK(hipMemcpy(&e, c->xerr, 4, hipMemcpyDeviceToHost));
        if (e) { (void)hipMemset(c->xerr, 0, 4); return fail("peer-to-peer exchange " + std::to_string(e - 1) + " timed out waiting for a peer (results of this call are invalid)"); }
    }
    if (!c->err || !(c->qkv_att || c->cls_tail)) return 0;
    if (!queued) HIP_OK(hipMemcpy(c->h_err, c->err, 4, hipMemcpyDeviceToHost));   // (queued: already copied by the stream, ahead of the synchronise the caller just did)
    if (*c->h_err) return fail("in-launch synchronisation timed out at stage " + std::to_string(*c->h_err - 1) + " (results of this call are invalid)");
    return 0;
}
// the end of every call that ran steps or passes: the error word's copy, the synchronise, the checks
int finish_call(lmrs_ctx* c) {
    if (queue_err(c)) return -1;
    HIP_OK(hipStreamSynchronize(c->stream));
    return check_err(c);
}

}  // namespace

extern "C" int lmrs_comm_unique_id(void* out128) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    if (!out128) return fail("out128 is NULL");
    ncclUniqueId id;
    NCCL_OK(ncclGetUniqueId(&id));
    memcpy(out128, &id, sizeof id);
    return 0;
}

static int create_impl(const uint8_t* file, size_t len, int device, int rank, int world, const void* uid, bool group_mode,
                       lmrs_ctx** out, size_t* bytes_consumed);

// Host-only: the row ranges shard `rank` of `world` owns.  plan[0..9] = q-head first/count, kv-head first/count,
// wo/w2 row first/count, gate-up pair first/count, classifier row first/count.  <0 if `world` does not divide the model.
extern "C" int lmrs_shard_plan(const lmrs_args* a, int rank, int world, int* plan) {
    if (!a || !plan || world < 1 || rank < 0 || rank >= world) return fail("bad argument");
    const Switches sw = read_switches();
    if (shard_plan_cls_only(*a, world, sw)) {                 // the layers whole on every shard, the classifier's rows split
        if (a->vocab_size % world) return fail("world must divide vocab_size");
        const int vl = a->vocab_size / world;
        const int p[10] = {0, (int)a->n_heads, 0, (int)a->n_kv_heads, 0, (int)a->dim, 0, (int)a->hidden_dim, rank * vl, vl};
        memcpy(plan, p, sizeof p);
        return 0;
    }
    if (a->n_kv_heads % world || a->dim % world || a->hidden_dim % world || a->vocab_size % world)
        return fail("world must divide n_kv_heads, dim, hidden_dim and vocab_size");
    const bool rep = !sw.shard_split_out;                     // wo / w2 rows: replicated on every shard by default
    const int nh = a->n_heads / world, nkv = a->n_kv_heads / world, dl = rep ? (int)a->dim : (int)a->dim / world, hl = a->hidden_dim / world, vl = a->vocab_size / world;
    const int p[10] = {rank * nh, nh, rank * nkv, nkv, rep ? 0 : rank * dl, dl, rank * hl, hl, rank * vl, vl};
    memcpy(plan, p, sizeof p);
    return 0;
}

// 1 if the sharded step of this context runs as one captured hipGraph (RCCL collectives inside), 0 if it is enqueued
// call by call, -1 if the context is not an RCCL shard.
extern "C" int lmrs_comm_ranks(const lmrs_ctx* c) {
    if (!c) return -1;
    if (!c->comm) return 0;
    int n = 0;
    return ncclCommCount(c->comm, &n) == ncclSuccess ? n : -1;
}
extern "C" int lmrs_shard_uses_graph(const lmrs_ctx* c) { return !c || !(c->comm || c->p2p) ? -1 : (primary_graph(c) ? 1 : 0); }

extern "C" int lmrs_create_sharded(const uint8_t* file, size_t len, int device, int rank, int world, const void* uid,
                                   lmrs_ctx** out, size_t* bytes_consumed) {
    if (world < 1 || rank < 0 || rank >= world) return fail("bad rank/world");
    // world > 1 without a communicator id: peer-to-peer transport, to be connected with lmrs_p2p_handle / lmrs_p2p_connect
    return create_impl(file, len, device, rank, world, uid, false, out, bytes_consumed);
}

extern "C" int lmrs_create(const uint8_t* file, size_t len, int device, lmrs_ctx** out, size_t* bytes_consumed) {
    return create_impl(file, len, device, 0, 1, nullptr, false, out, bytes_consumed);
}

// Verification aid (no reference counterpart): `world` row shards of one model as `world` contexts on ONE device,
// exchanged by device-to-device copies instead of RCCL, so that the sharding can be checked bit for bit on a
// single-GPU box.  shards[] receives `world` contexts; drive them with lmrs_group_forward.
extern "C" int lmrs_group_create(const uint8_t* file, size_t len, int device, int world, lmrs_ctx** shards, size_t* bytes_consumed) {
    if (world < 2 || !shards) return fail("a shard group needs world >= 2 (use lmrs_create for one GPU)");
    for (int r = 0; r < world; ++r) shards[r] = nullptr;
    for (int r = 0; r < world; ++r)
        if (create_impl(file, len, device, r, world, nullptr, true, &shards[r], bytes_consumed)) {
            for (int k = 0; k < r; ++k) { lmrs_destroy(shards[k]); shards[k] = nullptr; }
            return -1;
        }
    if (shards[0]->p2p) {                      // LMRS_GROUP_P2P=1: the shards exchange through the push kernel, concurrently on their own streams
        for (int r = 0; r < world; ++r) {
            for (int w = 0; w < world; ++w) shards[r]->peer_base[w] = shards[w]->xarena;
            shards[r]->p2p_ready = true;
        }
    }
    return 0;
}

// Peer-to-peer transport between PROCESSES (one per GPU): every rank exports the IPC handle of its exchange arena, the launcher
// distributes the `world` handles (any host transport), every rank connects.  No reference counterpart.
extern "C" int lmrs_p2p_handle(lmrs_ctx* c, void* out64) {
    if (!c || !out64) return fail("NULL argument");
    if (!c->p2p) return fail("not a peer-to-peer sharded context (create it with lmrs_create_sharded, world > 1, no communicator id)");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    HIP_OK(hipSetDevice(c->device));
    hipIpcMemHandle_t h;
    HIP_OK(hipIpcGetMemHandle(&h, c->xarena));
    memcpy(out64, &h, 64);
    return 0;
}
extern "C" int lmrs_p2p_connect(lmrs_ctx* c, const void* handles /* world x 64 bytes, in rank order */) {
    if (!c || !handles) return fail("NULL argument");
    if (!c->p2p) return fail("not a peer-to-peer sharded context");
    if (c->p2p_ready) return fail("already connected");
    if (c->inj_fail_connect) { c->inj_fail_connect = 0; return fail("peer-to-peer connect: injected failure (lmrs_debug_inject)"); }
    HIP_OK(hipSetDevice(c->device));
    for (int w = 0; w < c->world; ++w) {
        if (w == c->rank) continue;
        hipIpcMemHandle_t h; memcpy(&h, static_cast<const char*>(handles) + (size_t)w * 64, 64);
        void* p = nullptr;
        HIP_OK(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
        c->peer_base[w] = static_cast<char*>(p); c->xarena_is_ipc[w] = true;
    }
    c->p2p_ready = true;
    {   // handshake: one exchange of a rank-stamped block, so that a transport that does not work fails HERE, with a message
        float* probe = c->part;
        const float stamp = 1000.0f + (float)c->rank;
        HIP_OK(hipMemcpy(probe + (size_t)c->rank * 64, &stamp, 4, hipMemcpyHostToDevice));
        const ExchangeDesc e{reinterpret_cast<char*>(probe), 256, 256, nullptr, 0};
        c->ex_slot = kMaxExchangeSlots - 2;
        if (enqueue_exchange(c, e)) return -1;
        c->ex_slot = 0;
        HIP_OK(hipStreamSynchronize(c->stream));
        if (check_err(c)) return fail("peer-to-peer handshake: no flag from a peer within the timeout (are all ranks running, and can this GPU reach them?)");
        for (int w = 0; w < c->world; ++w) {
            float got = 0; HIP_OK(hipMemcpy(&got, probe + (size_t)w * 64, 4, hipMemcpyDeviceToHost));
            if (got != 1000.0f + (float)w) return fail("peer-to-peer handshake: the block of rank " + std::to_string(w) + " did not arrive");
        }
    }
    capture_sharded_step(c);
    return 0;
}

// One decode step over the shard group (segments in lockstep, slices exchanged by copies).  *logits (optional) = the
// assembled full logits on shard 0's pinned buffer; *next (optional) = the greedy token.
extern "C" int lmrs_group_forward(lmrs_ctx** sh, int world, uint32_t token, uint32_t pos, float** logits, uint32_t* next) {
    if (!sh || world < 1 || !sh[0]) return fail("bad argument");
    lmrs_ctx* c0 = sh[0];
    if (token >= c0->args.vocab_size) return fail("token out of range");
    if (pos >= c0->args.seq_len) return fail("pos out of range (seq_len is clamped to 8192)");
    HIP_OK(hipSetDevice(c0->device));
    for (int r = 0; r < world; ++r) {
        lmrs_ctx* c = sh[r];
        if (c->world != world || c->rank != r || c->comm || (c->p2p && !c->p2p_ready)) return fail("contexts are not a shard group made by lmrs_group_create");
        c->h_tok[0] = token;
        HIP_OK(hipMemcpyAsync(c->tokens + pos, c->h_tok, 4, hipMemcpyHostToDevice, c->stream));
        if (set_state(c, pos, 0)) return -1;
        HIP_OK(launch_embed(embed_args(c), c->stream));
    }
    const int ns = n_segments(c0);
    if (c0->p2p) {
        // every shard's whole step on its own stream, all in flight at once: the exchanges are the push kernels, the shards really
        // wait for each other on the device (as W processes on W GPUs would)
        for (int r = 0; r < world; ++r) if (enqueue_step_sharded(sh[r], StepForm{})) return -1;
        HIP_OK(hipDeviceSynchronize());
        for (int r = 0; r < world; ++r) if (check_err(sh[r])) return -1;
    } else
    for (int s = 0; s < ns; ++s) {
        for (int r = 0; r < world; ++r) if (run_segment(sh[r], StepForm{}, s)) return -1;
        HIP_OK(hipDeviceSynchronize());
        const ExchangeDesc g0 = exchange_after(c0, s);
        if (!g0.buf) continue;
        for (int dst = 0; dst < world; ++dst)
            for (int src = 0; src < world; ++src) {
                if (src == dst) continue;
                const ExchangeDesc gs = exchange_after(sh[src], s), gd = exchange_after(sh[dst], s);
                HIP_OK(hipMemcpyAsync(gd.buf + (size_t)src * gd.stride, gs.buf + (size_t)src * gs.stride, gs.bytes, hipMemcpyDeviceToDevice, sh[dst]->stream));
            }
        HIP_OK(hipDeviceSynchronize());
    }
    if (logits) {
        for (int r = 0; r < world; ++r)
            HIP_OK(hipMemcpyAsync(c0->h_logits + sh[r]->v0, sh[r]->logits + sh[r]->v0, (size_t)sh[r]->voc_l * 4, hipMemcpyDeviceToHost, c0->stream));
        *logits = c0->h_logits;
    }
    if (next) HIP_OK(hipMemcpyAsync(c0->h_tok + 1, c0->tokens + pos + 1, 4, hipMemcpyDeviceToHost, c0->stream));
    HIP_OK(hipDeviceSynchronize());
    if (next) *next = c0->h_tok[1];
    return 0;
}

static int create_impl(const uint8_t* file, size_t len, int device, int rank, int world, const void* uid, bool group_mode,
                       lmrs_ctx** out, size_t* bytes_consumed) {
    if (!out) return fail("out is NULL");
    *out = nullptr;
    Layout lay; std::string perr;
    if (!parse_layout(file, len, &lay, &perr)) return fail(perr);
    const Switches sw = read_switches();
    const lmrs_args& a = lay.args;
    const bool f32w = a.q_type == LMRS_Q_NONE;
    if (f32w && (world > 1 || uid)) return fail("q_type None (f32 weights) runs on one GPU only (row sharding is built for the quantised path)");
    if (!f32w && a.group_size != 128) return fail("group_size != 128 is not supported: export.py quantises with 128 whatever --group-size says and only writes the value into the header (utils/io.py:21), so such a file is not readable by the reference either");
    const size_t dim = a.dim, att = (size_t)a.n_heads * a.head_size, kv = (size_t)a.n_kv_heads * a.head_size, hid = a.hidden_dim, V = a.vocab_size;
    if (dim % 128 || att % 128 || hid % 128) return fail("dim, n_heads*head_size and hidden_dim must be multiples of 128");
    if (dim > 10240 || att > 10240 || hid > 16384) return fail("vector lengths above 10240 (dim, attention) / 16384 (hidden) are not supported");
    if (a.model_type == LMRS_PHI && a.head_size > 96)
        return fail("Phi: head_size above 96 indexes past the 48 LongRoPE short factors (transformer.rs:473-475: the reference panics)");
    if (a.head_size != 64 && a.head_size != 96 && a.head_size != 128 && a.head_size != 256) return fail("head_size must be 64, 96, 128 or 256 (the model families lm.rs supports)");
    int ndev = 0;
    hipError_t de = hipGetDeviceCount(&ndev);
    if (de != hipSuccess || ndev == 0) return fail("no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("bad device index");
    HIP_OK(hipSetDevice(device));

    // ---- shard plan: whole heads / rows per shard, equal sizes (in-place all-gathers need equal counts)
    const size_t W = (size_t)world;
    const bool cls_only = !f32w && shard_plan_cls_only(a, world, sw);
    if (cls_only ? V % W != 0 : world > 1 && (a.n_kv_heads % W || dim % W || hid % W || V % W))
        return fail(cls_only ? "world must divide vocab_size" : "world must divide n_kv_heads, dim, hidden_dim and vocab_size");
    if (a.vocab_size / (uint32_t)world < 4) return fail("vocab_size / world must be at least 4");
    const size_t hs = a.head_size;
    // wo and w2 (the projections back to the residual stream) are REPLICATED by default: every shard computes all dim rows
    // from the gathered att_out / h, so the residual needs no gather of its own - two all-gathers per layer instead of four,
    // for 4 + 17 MB of extra weight reads per layer and shard (1-3 us) against two ~10-20 us latency-bound collectives.
    // LMRS_SHARD_SPLIT_OUT=1 restores the fully row-split form.
    const bool rep_out = cls_only || !sw.shard_split_out;
    const size_t WL = cls_only ? 1 : W;                                 // the layers' split ("cls": none)
    const size_t att_l = att / WL, kv_l = kv / WL, dim_l = rep_out ? dim : dim / W, hid_l = hid / WL, voc_l = V / W;
    const size_t a0 = cls_only ? 0 : rank * att_l, k0 = cls_only ? 0 : rank * kv_l, d0 = rep_out ? 0 : rank * dim_l, h0 = cls_only ? 0 : rank * hid_l, v0 = rank * voc_l;
    (void)hs;

    lmrs_ctx* c = new lmrs_ctx();
    c->sw = sw;
    c->args = a; c->lay = lay; c->device = device; c->q4 = a.q_type == LMRS_Q4_0; c->f32 = f32w;
    c->rank = rank; c->world = world; c->att_full = (int)att;
    c->att_dim = (int)att_l; c->kv_dim = (int)kv_l; c->dim_l = (int)dim_l; c->hid_l = (int)hid_l; c->voc_l = (int)voc_l;
    c->a0 = (int)a0; c->d0 = (int)d0; c->h0 = (int)h0; c->v0 = (int)v0;
    c->rep_out = rep_out; c->cls_only = cls_only;
    const bool sharded = world > 1 || uid != nullptr;
    // transport of the exchanges: RCCL when a communicator id is given; otherwise peer-to-peer pushes (separate processes
    // connect through lmrs_p2p_handles / lmrs_p2p_connect; a lock-step group on one device uses plain copies unless LMRS_GROUP_P2P=1)
    c->p2p = sharded && world > 1 && !uid && (!group_mode || sw.group_p2p);
    if (c->p2p && world > kMaxWorld) { delete c; return fail("the peer-to-peer transport connects at most " + std::to_string(kMaxWorld) + " shards (the GPUs of one node): pass a communicator id (RCCL) for larger worlds"); }
    auto cleanup = [&]() { lmrs_destroy(c); return -1; };
#define CK(call) do { if ((call)) return cleanup(); } while (0)
#define HCK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { fail(std::string(#expr) + ": " + hipGetErrorString(e_)); return cleanup(); } } while (0)
    HCK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HCK(hipEventCreate(&c->ev0)); HCK(hipEventCreate(&c->ev1));
    if (sharded && !group_mode && uid) {
        ncclUniqueId id; memcpy(&id, uid, sizeof id);
        ncclResult_t nr = ncclCommInitRank(&c->comm, world, id, rank);
        if (nr != ncclSuccess) { fail(std::string("ncclCommInitRank: ") + ncclGetErrorString(nr)); return cleanup(); }
    }

    const size_t G = 128, bpe_num = f32w ? 8 : (c->q4 ? 1 : 2);   // bytes per element = bpe_num / 2 (f32 weights: 4, no scales)
    auto qbytes = [&](size_t rows, size_t cols) { return rows * cols * bpe_num / 2; };
    auto sbytes = [&](size_t rows, size_t cols) { return f32w ? (size_t)0 : rows * cols / G * 4; };
    const size_t nl = a.n_layers;
    size_t total = 0;
    auto need = [&](size_t b) { total += pad256(b); };
    for (size_t l = 0; l < nl; ++l) {
        need(qbytes(att_l + 2 * kv_l, dim)); need(sbytes(att_l + 2 * kv_l, dim));
        need(qbytes(dim_l, att)); need(sbytes(dim_l, att));
        need(qbytes(2 * hid_l, dim)); need(sbytes(2 * hid_l, dim));
        need(qbytes(dim_l, hid)); need(sbytes(dim_l, hid));
        for (int i = 0; i < 4; ++i) need(dim * 4);
    }
    need(qbytes(V, dim)); need(sbytes(V, dim));
    if (a.model_type == LMRS_PHI) { need(qbytes(V, dim)); need(sbytes(V, dim)); }
    need(dim * 4);
    const size_t kvn = nl * a.seq_len * kv_l;
    need(kvn * 4); need(kvn * 4);
    need((size_t)a.seq_len * a.head_size * 4);                               // rope table
    need(dim * 4); need(att_l * 4); need(kv_l * 4); need(att * 4); need(hid * 4); need(V * 4); need(dim * 4); need(dim * 4);
    need(kMaxArgmaxParts * 4); need(kMaxArgmaxParts * 4); need(W * 2 * kMaxArgmaxParts * 4);
    // quantised exchange payloads (Q8_0, whole 128-groups per shard): one padded block per shard
    c->qpay = sharded && !cls_only && !c->q4 && att_l % 128 == 0 && hid_l % 128 == 0 && !sw.shard_f32_payload;
    c->tp_prefill = sharded && prefill_tp_shapes_ok(c);
    c->blk_att = pad256(att_l + att_l / 32); c->blk_h = pad256(hid_l + hid_l / 32);
    need(W * c->blk_att); need(W * c->blk_h);
    need(((size_t)a.seq_len + 8) * 4); need(sizeof(DevState));
    c->stage_floats = 64 * dim; need(c->stage_floats * 4); need(64 * 4); need(8 * 1024 * 8); need(512);
    need(nl * (att / 4 + att / 128) * 8);                                              // granules of the three-part launch
    need(nl * dim * 8);                                                                // granules of the wo + w1/w3 launch
    need(nl * (att_l + 2 * kv_l) * 8); need(256); need(256); need(256); need(kMaxArgmaxParts * 8); need(256);       // granules of the merged qkv + attention launch, step sequence number, error word
    total += 4096;
    HCK(hipMalloc(reinterpret_cast<void**>(&c->arena), total));
    c->arena_bytes = total;

    // ---- weights: this shard's rows only (the embedding / classifier table stays whole: any row may be looked up)
    auto upload_rows = [&](void* dst, const TensorView& tv, size_t row0, size_t nrows, size_t cols, bool scales) -> int {
        if (scales && f32w) return 0;
        const size_t rb = scales ? cols / G * 4 : qbytes(1, cols);
        return upload(c, dst, file + (scales ? tv.s_off : tv.q_off) + row0 * rb, nrows * rb);
    };
    c->layers.resize(nl);
    for (size_t l = 0; l < nl; ++l) {
        DevLayer& D = c->layers[l];
        char* wqkv = c->alloc<char>(qbytes(att_l + 2 * kv_l, dim)); float* sqkv = c->alloc<float>(sbytes(att_l + 2 * kv_l, dim) / 4);
        char* wo = c->alloc<char>(qbytes(dim_l, att)); float* so = c->alloc<float>(sbytes(dim_l, att) / 4);
        char* w13 = c->alloc<char>(qbytes(2 * hid_l, dim)); float* s13 = c->alloc<float>(sbytes(2 * hid_l, dim) / 4);
        char* w2 = c->alloc<char>(qbytes(dim_l, hid)); float* s2 = c->alloc<float>(sbytes(dim_l, hid) / 4);
        float* r0 = c->alloc<float>(dim); float* r1 = c->alloc<float>(dim); float* r2 = c->alloc<float>(dim); float* r3 = c->alloc<float>(dim);
        if (!wqkv || !sqkv || !wo || !so || !w13 || !s13 || !w2 || !s2 || !r3) { fail("arena overflow"); return cleanup(); }
        const TensorView &tq = lay.wq[l], &tk = lay.wk[l], &tv = lay.wv[l];
        const size_t rb = qbytes(1, dim), srb = dim / G * 4;
        CK(upload_rows(wqkv, tq, a0, att_l, dim, false));
        CK(upload_rows(wqkv + att_l * rb, tk, k0, kv_l, dim, false));
        CK(upload_rows(wqkv + (att_l + kv_l) * rb, tv, k0, kv_l, dim, false));
        CK(upload_rows(sqkv, tq, a0, att_l, dim, true));
        CK(upload_rows(reinterpret_cast<char*>(sqkv) + att_l * srb, tk, k0, kv_l, dim, true));
        CK(upload_rows(reinterpret_cast<char*>(sqkv) + (att_l + kv_l) * srb, tv, k0, kv_l, dim, true));
        CK(upload_rows(wo, lay.wo[l], d0, dim_l, att, false));
        CK(upload_rows(so, lay.wo[l], d0, dim_l, att, true));
        CK(upload_interleaved(c, w13, file + lay.w1[l].q_off + h0 * rb, rb, hid_l, 0));
        CK(upload_interleaved(c, w13, file + lay.w3[l].q_off + h0 * rb, rb, hid_l, 1));
        if (!f32w) { CK(upload_interleaved(c, s13, file + lay.w1[l].s_off + h0 * srb, srb, hid_l, 0)); CK(upload_interleaved(c, s13, file + lay.w3[l].s_off + h0 * srb, srb, hid_l, 1)); }
        CK(upload_rows(w2, lay.w2[l], d0, dim_l, hid, false));
        CK(upload_rows(s2, lay.w2[l], d0, dim_l, hid, true));
        CK(upload(c, r0, file + lay.rms_att[l].q_off, dim * 4));
        CK(upload(c, r1, file + lay.rms_post_att[l].q_off, dim * 4));
        if (a.model_type == LMRS_GEMMA) {
            CK(upload(c, r2, file + lay.rms_pre_ffn[l].q_off, dim * 4));
            CK(upload(c, r3, file + lay.rms_post_ffn[l].q_off, dim * 4));
        }
        D.wqkv = wqkv; D.sqkv = sqkv; D.wo = wo; D.so = so; D.w13 = w13; D.s13 = s13; D.w2 = w2; D.s2 = s2;
        D.rms_att = r0; D.rms_post_att = r1; D.rms_pre_ffn = r2; D.rms_post_ffn = r3;
    }
    {
        char* eq = c->alloc<char>(lay.emb.q_bytes); float* es = c->alloc<float>(lay.emb.s_bytes / 4);
        if (!eq || !es) { fail("arena overflow"); return cleanup(); }
        CK(upload(c, eq, file + lay.emb.q_off, lay.emb.q_bytes)); if (!f32w) CK(upload(c, es, file + lay.emb.s_off, lay.emb.s_bytes));
        c->emb_q = eq; c->emb_s = es; c->cls_q = eq; c->cls_s = es;        // tied classifier = the QUANTISED table
        if (a.model_type == LMRS_PHI) {
            char* hq = c->alloc<char>(lay.lm_head.q_bytes); float* hsx = c->alloc<float>(lay.lm_head.s_bytes / 4);
            if (!hq || !hsx) { fail("arena overflow"); return cleanup(); }
            CK(upload(c, hq, file + lay.lm_head.q_off, lay.lm_head.q_bytes)); if (!f32w) CK(upload(c, hsx, file + lay.lm_head.s_off, lay.lm_head.s_bytes));
            c->cls_q = hq; c->cls_s = hsx;
        }
        float* rf = c->alloc<float>(dim);
        CK(upload(c, rf, file + lay.rms_final.q_off, dim * 4));
        c->rms_final = rf;
    }
    // ---- state
    c->k_cache = c->alloc<float>(kvn); c->v_cache = c->alloc<float>(kvn);
    c->rope = c->alloc<float>((size_t)a.seq_len * a.head_size);
    c->x = c->alloc<float>(dim); c->q = c->alloc<float>(att_l); c->k_raw = c->alloc<float>(kv_l); c->x2 = c->alloc<float>(dim);
    c->part_val = c->alloc<float>(kMaxArgmaxParts); c->part_idx = c->alloc<int>(kMaxArgmaxParts);
    if (c->p2p) {
        // every buffer a peer writes into: one fine-grained (L2-uncached, system-coherent) allocation, same layout on every shard
        size_t xo = 0;
        auto xneed = [&](size_t b) { const size_t o = xo; xo += pad256(b); return o; };
        const size_t o_att = xneed(att * 4), o_h = xneed(hid * 4), o_tmp = xneed(dim * 4), o_logits = xneed(V * 4), o_part = xneed(2 * W * 2 * kMaxArgmaxParts * 4),
                     o_gqa = xneed(W * c->blk_att), o_gqh = xneed(W * c->blk_h), o_flags = xneed((size_t)kMaxExchangeSlots * kMaxWorld * 4), o_seq = xneed((size_t)kMaxExchangeSlots * 4), o_err = xneed(256);
        const bool tpb = c->tp_prefill;                       // token-batch blocks of the batched prefill (two buffers: see prefill_layers)
        c->pfb_att = prefill_tp_block(att_l); c->pfb_h = prefill_tp_block(hid_l); c->pfb_x = pad256((size_t)kPrefillTokens * dim_l * 4);
        const size_t o_pfa = tpb ? xneed(W * c->pfb_att) : 0, o_pfh = tpb ? xneed(W * c->pfb_h) : 0, o_pfx = tpb && !rep_out ? xneed(W * c->pfb_x) : 0;
        HCK(hipExtMallocWithFlags(reinterpret_cast<void**>(&c->xarena), xo, hipDeviceMallocFinegrained));
        c->xarena_bytes = xo;
        HCK(hipMemset(c->xarena, 0, xo));
        c->att_out = reinterpret_cast<float*>(c->xarena + o_att); c->h = reinterpret_cast<float*>(c->xarena + o_h); c->tmp = reinterpret_cast<float*>(c->xarena + o_tmp);
        c->logits = reinterpret_cast<float*>(c->xarena + o_logits); c->part = reinterpret_cast<float*>(c->xarena + o_part);
        c->gq_att = c->xarena + o_gqa; c->gq_h = c->xarena + o_gqh;
        if (tpb) { c->pfx_att = c->xarena + o_pfa; c->pfx_h = c->xarena + o_pfh; if (!rep_out) c->pfx_x = c->xarena + o_pfx; }
        c->xflags = reinterpret_cast<unsigned*>(c->xarena + o_flags); c->xseq = reinterpret_cast<unsigned*>(c->xarena + o_seq); c->xerr = reinterpret_cast<int*>(c->xarena + o_err);
        c->peer_base[rank] = c->xarena;
        if (cls_only) {   // no peer ever writes the layers' activations: they belong in ordinary (L2-cached) memory; only the partials and logits are exchanged
            c->att_out = c->alloc<float>(att); c->h = c->alloc<float>(hid); c->tmp = c->alloc<float>(dim);
        }
    } else {
        c->att_out = c->alloc<float>(att); c->h = c->alloc<float>(hid); c->logits = c->alloc<float>(V); c->tmp = c->alloc<float>(dim);
        c->part = c->alloc<float>(W * 2 * kMaxArgmaxParts);
        c->gq_att = c->alloc<char>(W * c->blk_att); c->gq_h = c->alloc<char>(W * c->blk_h);
    }
    c->tokens = c->alloc<uint32_t>((size_t)a.seq_len + 8); c->st = c->alloc<DevState>(1);
    c->seq = c->alloc<unsigned>(1); c->cls_seq = c->alloc<unsigned>(1); c->gran = c->alloc<unsigned long long>(nl * (att_l + 2 * kv_l)); c->err = c->alloc<int>(1);
    c->part_pk = c->alloc<unsigned long long>(kMaxArgmaxParts);
    if (!c->seq || !c->cls_seq || !c->gran || !c->err || !c->part_pk) { fail("arena overflow"); return cleanup(); }
    HCK(hipMemsetAsync(c->part_pk, 0, kMaxArgmaxParts * 8, c->stream));
    HCK(hipMemsetAsync(c->seq, 0, 4, c->stream)); HCK(hipMemsetAsync(c->cls_seq, 0, 4, c->stream)); HCK(hipMemsetAsync(c->gran, 0, nl * (att_l + 2 * kv_l) * 8, c->stream)); HCK(hipMemsetAsync(c->err, 0, 4, c->stream));
    if (sw.debug_timeline) { c->dbg = c->alloc<unsigned long long>(8 * 1024); if (c->dbg) HCK(hipMemsetAsync(c->dbg, 0, 8 * 1024 * 8, c->stream)); }
    c->stage = c->alloc<float>(c->stage_floats);
    if (!c->stage) { fail("arena overflow"); return cleanup(); }
    HCK(hipMemsetAsync(c->k_cache, 0, kvn * 4, c->stream)); HCK(hipMemsetAsync(c->v_cache, 0, kvn * 4, c->stream));   // :302-303
    HCK(hipMemsetAsync(c->tokens, 0, ((size_t)a.seq_len + 8) * 4, c->stream));
    HCK(hipMemsetAsync(c->logits, 0, V * 4, c->stream));
    {
        const uint32_t half = a.head_size / 2;
        std::vector<float> tab((size_t)a.seq_len * a.head_size);
        for (uint32_t p = 0; p < a.seq_len; ++p)
            for (uint32_t j = 0; j < half; ++j) rope_terms(a, p, j, &tab[((size_t)p * half + j) * 2], &tab[((size_t)p * half + j) * 2 + 1]);
        HCK(hipMemcpyAsync(c->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
        HCK(hipStreamSynchronize(c->stream));       // tab goes out of scope
    }
    if (!alloc_all({{c->h_logits, V}, {c->h_tok, (size_t)a.seq_len + 8}, {c->h_st, kStateSlots}, {c->h_err, 1}})) { alloc_failed("pinned host buffers: hipHostMalloc"); return cleanup(); }
    CK(set_state(c, 0, 0));
    HCK(hipStreamSynchronize(c->stream));
    if (a.model_type == LMRS_GEMMA && !sharded && !f32w) {
        // fold the two "x += rmsnorm(branch)" steps of a Gemma layer into the consuming GEMV prologues when every launch of the
        // step has a static kernel that can do it (otherwise: the separate addnorm launches)
        GemvArgs q{}; q.q4 = c->q4; q.n = a.dim; q.o = c->att_dim + 2 * c->kv_dim;
        GemvArgs f = q; f.o = 2 * a.hidden_dim;
        GemvArgs k = q; k.o = cls_rows(c); k.softcap_rows = (int)a.dim;
        c->gemma_fused = gemv_is_static(q, PRO_ADD_RMS_QUANT, EPI_QKV) && gemv_is_static(f, PRO_ADD_RMS_QUANT, EPI_GELU) &&
                         gemv_is_static(k, PRO_ADD_RMS_QUANT, EPI_CLS);
    }
    {
        GemvArgs g = cls_args(c);
        c->cls_grid = f32w ? gemv_f32_grid(g, EPI_CLS) : gemv_grid(g, c->gemma_fused ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT, EPI_CLS);
        c->part_stride = (2 * c->cls_grid + 3) & ~3;
    }
    // (also the "cls" shard plan in its one-process-per-GPU form: there every GPU runs the layers whole, with the single-GPU launches)
    if ((!sharded || (cls_only && !group_mode)) && !f32w && sw.qkv_att != 0) {
        // qkv + attention as one launch (short contexts) when the model's qkv launch has a merged class for every prologue it uses
        GemvArgs q{}; q.q4 = c->q4; q.n = a.dim; q.o = c->att_dim + 2 * c->kv_dim;
        AttnArgs t{}; t.n_heads = a.n_heads; t.n_kv_heads = a.n_kv_heads; t.head_size = a.head_size; t.gemma = a.model_type == LMRS_GEMMA;
        c->qkv_att = qkv_attn_supported(q, PRO_RMS_QUANT, t) && (!c->gemma_fused || qkv_attn_supported(q, PRO_ADD_RMS_QUANT, t)) &&
                     !(a.model_type == LMRS_GEMMA && !c->gemma_fused);
        c->qa_max_T = a.seq_len < 1024 ? (int)a.seq_len : 1024;
        if (c->qkv_att && sw.qkv_att != 1) c->qa_wave_T = qkv_attn_wave_T((int)a.head_size);   // LMRS_QKV_ATT=1: workgroup form only
        // (the wave forms' prefetch reads whole 64-row blocks of the caches - 128 rows for the 64-wide heads; their form for positions 128 .. 255 clamps its rows to the sequence)
        if (c->qa_wave_T > (int)a.seq_len) c->qa_wave_T = a.head_size == 64 && a.seq_len >= 128 ? (int)a.seq_len : 0;
    }
    c->split_merged = c->qkv_att && !sharded && sw.att_split_merged;      // (sharded contexts and f32 files: the split form stays six launches)
    if (!sharded) c->multi_k = sw.steps_per_graph;   // (measured: 4 steps per launch +1.5 % on a 20-step run, no effect on long runs)
    c->cls_tail = !sharded && !f32w && V < (1u << 20) - 1 && sw.cls_tail;
    if (!sharded) {
        CK(!step_graph(c, step_form_for(c, 0)));
        CK(capture(c, StepForm{}, false, &c->g_layers));      // (fill_kv_cache's token-by-token form at ANY position: the separate kernels)
        // from this position on a step uses the split attention (scores by key chunk, V by dim slice): graphs captured on first use
        if (!c->dbg || sw.att_split_pos_set) c->att_split_pos = sw.att_split_pos;     // (stamped steps: the split form only when asked for)
        // every graph a call below that threshold can need - per qkv + attention mode the single-step graph and the multi-step one -
        // is captured here rather than inside the first generate call that reaches the mode (a capture is milliseconds: on a
        // 128-token run that crosses the wave -> workgroup switch it was 3 % of the run)
        if (!c->dbg && c->qkv_att) {
            for (int mode = 1; mode <= 2; ++mode) {
                if (mode == 2 && c->qa_wave_T <= 0) continue;
                if (mode == 1 && c->qa_wave_T >= c->qa_max_T) continue;
                CK(!step_graph(c, StepForm{mode, 0}));
                if (c->multi_k > 1) CK(!step_graph(c, StepForm{mode, 0}, c->multi_k));
            }
        }
    } else if (c->comm) {
        // RCCL collectives inside a captured graph: use it when the runtime accepts it, else enqueue every step
        capture_sharded_step(c);
    }
    // (peer-to-peer contexts capture their step graph in lmrs_p2p_connect, once the peers' arenas are known)
    if (sharded) c->att_split_pos = sw.att_split_pos;
    // Row shards over RCCL whose prefill is batched allocate its buffers (the token-batch blocks of the all-gathers among them) HERE: a shard
    // that failed to allocate them inside its first fill_kv_cache would return before the exchange its peers are already waiting in
    // (ncclAllGather has no time-out); at create the failure surfaces on every rank's own call, before any exchange exists.
    if (c->tp_prefill && c->comm && (c->world > 1 || c->comm) && !c->cls_only) CK(prefill_alloc(c));
#undef CK
#undef HCK
    *out = c;
    if (bytes_consumed) *bytes_consumed = lay.end;
    return 0;
}

// What is not plain memory goes here, in this order; the context's owners (lmrs_buf.h) free theirs in `delete c`, on the context's device
extern "C" void lmrs_destroy(lmrs_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    destroy_step_graphs(c);
    if (c->g_layers) (void)hipGraphExecDestroy(c->g_layers);
    if (c->pfx_owned) { if (c->pfx_att) (void)hipFree(c->pfx_att); if (c->pfx_h) (void)hipFree(c->pfx_h); if (c->pfx_x) (void)hipFree(c->pfx_x); }
    if (c->comm) ncclCommDestroy(c->comm);
    for (int w = 0; w < kMaxWorld; ++w) if (c->xarena_is_ipc[w] && c->peer_base[w]) (void)hipIpcCloseMemHandle(c->peer_base[w]);
    if (c->xarena) (void)hipFree(c->xarena);
    if (c->arena) (void)hipFree(c->arena);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" const lmrs_args* lmrs_get_args(const lmrs_ctx* c) { return c ? &c->args : nullptr; }

// one decode step on the context's stream: the replay of its form's graph, or eager launches
static int launch_step(lmrs_ctx* c, uint32_t pos) {
    const bool sharded = c->comm || c->p2p;
    if (c->p2p && !c->p2p_ready) return fail("peer-to-peer transport: peers not connected yet (lmrs_p2p_connect)");
    if (sharded && c->world > 1 && !c->comm && !c->p2p) return fail("this context is a member of a lock-step shard group: drive it with lmrs_group_forward");
    // Eager: a sharded step whose exchanges the runtime refused to capture (it runs the separate kernels), and the profiling aid LMRS_NO_GRAPH=1 - the
    // launches of the graph enqueued one by one: rocprofv3 1.1's dispatch interceptor segfaults on the graph launches of every model but Llama-3.2-1B
    // (profiles/README.md); token ids are the same either way
    const bool graphs = primary_graph(c) != nullptr, eager = graphs ? c->sw.no_graph && !sharded : sharded && c->eager;
    const StepForm f = step_form_for(c, pos, /*merged=*/graphs);
    if (split_scratch(c, f)) return -1;
    if (!graphs && !eager) return fail("this context is a member of a lock-step shard group: drive it with lmrs_group_forward");
    if (!eager) return replay_steps(c, f);
    c->dbg_node = 0;
    return sharded ? enqueue_step_sharded(c, f) : enqueue_step(c, f);
}

static int step_once(lmrs_ctx* c, uint32_t token, uint32_t pos) {
    if (!c) return fail("ctx is NULL");
    if (token >= c->args.vocab_size) return fail("token out of range");
    if (pos >= c->args.seq_len) return fail("pos out of range (seq_len is clamped to 8192)");
    HIP_OK(hipSetDevice(c->device));
    c->h_tok[0] = token;
    HIP_OK(hipMemcpyAsync(c->tokens + pos, c->h_tok, 4, hipMemcpyHostToDevice, c->stream));
    if (set_state(c, pos, 0)) return -1;
    HIP_OK(launch_embed(embed_args(c), c->stream));
    return launch_step(c, pos);
}

extern "C" int lmrs_forward(lmrs_ctx* c, uint32_t token, uint32_t pos, float** logits) {
    if (step_once(c, token, pos)) return -1;
    if (c->world > 1) {                                        // every shard returns the whole logits vector
        const ExchangeDesc e{reinterpret_cast<char*>(c->logits), (size_t)c->voc_l * 4, (size_t)c->voc_l * 4, nullptr, 0};
        const int keep = c->ex_slot; c->ex_slot = kMaxExchangeSlots - 1;      // a slot of its own: the step graph's slots were fixed at capture
        const int rc = enqueue_exchange(c, e);
        c->ex_slot = keep;
        if (rc) return -1;
    }
    HIP_OK(hipMemcpyAsync(c->h_logits, c->logits, (size_t)c->args.vocab_size * 4, hipMemcpyDeviceToHost, c->stream));
    if (finish_call(c)) return -1;
    if (logits) *logits = c->h_logits;
    return 0;
}

extern "C" int lmrs_forward_argmax(lmrs_ctx* c, uint32_t token, uint32_t pos, uint32_t* next) {
    if (step_once(c, token, pos)) return -1;
    HIP_OK(hipMemcpyAsync(c->h_tok + 1, c->tokens + pos + 1, 4, hipMemcpyDeviceToHost, c->stream));
    if (finish_call(c)) return -1;
    if (next) *next = c->h_tok[1];
    return 0;
}

// the device sort's buffers (launch_sample_topp_sort): keys, the count word behind them, the sorted pairs and their pinned copy - once, for the whole
// vocabulary of n entries, at the first call that sorts N keys
static int samp_sort_alloc(lmrs_ctx* c, int N, size_t n) {
    if (c->samp_cap >= N) return 0;
    int cap = sample_sort_min_n();
    while ((size_t)cap < n) cap <<= 1;                                               // once, for the whole vocabulary
    c->samp_cap = 0;
    if (!alloc_all({{c->samp_keys, (size_t)cap + 32}, {c->samp_pairs, (size_t)cap * 2}, {c->h_pairs, (size_t)cap * 8 + 8}})) return alloc_failed("top-p sort buffers: hipMalloc");
    c->samp_cap = cap;
    return 0;
}
struct lmrs_sampler;
extern "C" int lmrs_sampler_info(const lmrs_sampler* s, uint32_t* vocab_size, float* temperature, float* top_p, float* rnd);
extern "C" int lmrs_sampler_sample(lmrs_sampler* s, float* logits, uint32_t* next);
extern "C" int lmrs_sampler_sample_exps(lmrs_sampler* s, float* exps, uint32_t* next);
extern "C" int lmrs_forward_sample(lmrs_ctx* c, uint32_t token, uint32_t pos, lmrs_sampler* sampler, uint32_t* next) {
    if (!c || !sampler || !next) return fail("NULL argument");
    uint32_t vs = 0; float temp = 0, top_p = 0, rnd = 0;
    if (lmrs_sampler_info(sampler, &vs, &temp, &top_p, &rnd)) return -1;
    if (vs != c->args.vocab_size) return fail("the sampler was made for another vocabulary size");
    if (temp == 0.0f) return lmrs_forward_argmax(c, token, pos, next);                    // sample_argmax: fused into the step
    if (c->world > 1 || c->comm) {                                                        // sharded logits: the host sampler
        float* lg = nullptr;
        if (lmrs_forward(c, token, pos, &lg)) return -1;
        return lmrs_sampler_sample(sampler, lg, next);
    }
    // temperature != 0: the parallel part on the device (scaling, maximum, exponentials), the sequential chains on the host (lmrs_sampler_sample_exps)
    (void)top_p; (void)rnd;
    if (step_once(c, token, pos)) return -1;
    const size_t n = c->args.vocab_size;
    SampleArgs sa{c->logits, (int)n, temp, c->part_val};                                  // (scratch: the argmax partials)
    HIP_OK(launch_sample_exps(sa, c->stream));
    HIP_OK(hipMemcpyAsync(c->h_logits, c->logits, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (finish_call(c)) return -1;
    // the sequential sum, the division and the cutoff filter on the host (lmrs_text.cpp); the exponentials are still in c->logits on the device
    float sum = 0.0f, cutoff = 0.0f; size_t n0 = 0;
    if (lmrs_sampler_exps_prepare(sampler, c->h_logits, &sum, &cutoff, &n0)) return -1;
    if (n0 < c->sw.topp_sort_min || !(sum == sum)) return lmrs_sampler_exps_finish(sampler, c->h_logits, nullptr, next);
    // many candidates (a flat distribution): their sort (sampler.rs:81) on the device - probabilities re-formed there from the same exponentials and
    // the same sum by the same IEEE division, so the device finds the same n0 candidates (checked) - and only the sorted pairs come back
    int N = sample_sort_min_n();
    while ((size_t)N < n0) N <<= 1;
    if (samp_sort_alloc(c, N, n)) return -1;
    unsigned* count = reinterpret_cast<unsigned*>(c->samp_keys + c->samp_cap);           // (the word behind the keys)
    HIP_OK(launch_sample_topp_sort(c->logits, (int)n, sum, cutoff, N, c->samp_keys, count, c->samp_pairs, c->stream));
    HIP_OK(hipMemcpyAsync(c->h_pairs, c->samp_pairs, n0 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(c->h_pairs + (size_t)c->samp_cap * 8, count, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    unsigned dev_n0 = 0; memcpy(&dev_n0, c->h_pairs + (size_t)c->samp_cap * 8, 4);
    if (dev_n0 != n0) return fail("lmrs_forward_sample: the device found " + std::to_string(dev_n0) + " top-p candidates, the host " + std::to_string(n0));
    return lmrs_sampler_exps_finish(sampler, c->h_logits, c->h_pairs, next);
}

extern "C" int lmrs_get_embeddings(const lmrs_ctx* cc, const uint32_t* tokens, size_t n, float* out) {
    lmrs_ctx* c = const_cast<lmrs_ctx*>(cc);
    if (!c || !tokens || !out) return fail("NULL argument");
    HIP_OK(hipSetDevice(c->device));
    const size_t dim = c->args.dim, chunk = c->stage_floats / dim < 64 ? c->stage_floats / dim : 64;
    uint32_t* dtok = reinterpret_cast<uint32_t*>(c->stage + c->stage_floats);   // 64 ints after the staging floats
    for (size_t i0 = 0; i0 < n; i0 += chunk) {
        const size_t m = n - i0 < chunk ? n - i0 : chunk;
        for (size_t i = 0; i < m; ++i) if (tokens[i0 + i] >= c->args.vocab_size) return fail("token out of range");
        HIP_OK(hipMemcpyAsync(dtok, tokens + i0, m * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(launch_dequant_rows(c->emb_q, c->emb_s, c->f32 ? 2 : (int)c->q4, dtok, (int)m, (int)dim, c->stage, c->stream));
        HIP_OK(hipMemcpyAsync(out + i0 * dim, c->stage, m * dim * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// ------------------------------------------------------------------ batched forward_layer on the matrix cores

// The model shapes the static per-token prologues exist for (Llama-3.2-1B/3B, Phi-3.5, Gemma-2-2B; Q8_0 and Q4_0) on one GPU;
// everything else takes the token-by-token path below (same results).
static bool prefill_batched_ok(const lmrs_ctx* c) {
    const lmrs_args& a = c->args;
    if (c->sw.no_batched_prefill) return false;
    // (a "cls" shard runs the layers whole: the batched path applies to it as to a single GPU, every shard filling its own cache)
    const bool whole_layers = c->cls_only || (c->world == 1 && !c->comm && c->g_layers);
    if ((a.q_type != LMRS_Q8_0 && a.q_type != LMRS_Q4_0) || !whole_layers) return false;
    if (!rows_prologue_supported((int)a.dim) || !rows_prologue_supported(c->att_dim) || !rows_prologue_supported((int)a.hidden_dim)) return false;
    if (a.model_type == LMRS_GEMMA) { if (a.head_size != 256 || a.dim != 2304) return false; }
    else if (a.head_size != 64 && a.head_size != 96 && a.head_size != 128) return false;
    return (c->att_dim + 2 * c->kv_dim) % 16 == 0 && c->kv_dim % 4 == 0 && a.dim % 16 == 0;
}

static int prefill_alloc(lmrs_ctx* c) {
    if (c->pf_ready) return 0;
    const lmrs_args& a = c->args;
    const size_t B = kPrefillTokens, wide = std::max<size_t>(std::max<size_t>(a.dim, a.hidden_dim), (size_t)std::max(c->att_dim, c->att_full));
    const bool own_blocks = c->tp_prefill && c->comm && !c->pfx_att;      // (peer-to-peer shards: the blocks are part of the exchange arena, laid out at create)
    if (own_blocks) { c->pfb_att = prefill_tp_block((size_t)c->att_dim); c->pfb_h = prefill_tp_block((size_t)c->hid_l); c->pfb_x = pad256((size_t)kPrefillTokens * c->dim_l * 4); c->pfx_owned = true; }
    // all or nothing (alloc_all), Gemma's pf_t and the shards' own blocks with the set: the blocks stay raw pointers - on peer-to-peer shards they are
    // views into the exchange arena
    struct Want { char** p; size_t bytes; } blocks[] = {{&c->pfx_att, c->world * c->pfb_att}, {&c->pfx_h, c->world * c->pfb_h}, {&c->pfx_x, c->rep_out ? 0 : c->world * c->pfb_x}};
    bool ok = alloc_all({{c->pf_x, B * a.dim}, {c->pf_q, B * c->att_dim}, {c->pf_k, B * c->kv_dim}, {c->pf_ao, B * c->att_dim}, {c->pf_h, B * a.hidden_dim}, {c->pf_xq, B * wide},
                         {c->pf_xs, B * (wide / 128)}}) && (a.model_type != LMRS_GEMMA || c->pf_t.alloc(B * a.dim));
    for (const Want& w : blocks) if (ok && own_blocks && w.bytes) ok = (*w.p = static_cast<char*>(DevMem::obtain(w.bytes))) != nullptr;
    if (!ok) {
        c->pf_x.reset(); c->pf_q.reset(); c->pf_k.reset(); c->pf_ao.reset(); c->pf_h.reset(); c->pf_xq.reset(); c->pf_xs.reset(); c->pf_t.reset();
        for (const Want& w : blocks) if (own_blocks && *w.p) { DevMem::release(*w.p); *w.p = nullptr; }
        return alloc_failed("prefill buffers: hipMalloc");
    }
    // The layers' weight scales transposed, [group][row], once: a ring GEMM fetches a group's scales of 64 rows as 256 consecutive bytes instead of 4 bytes
    // from each of 64 lines (GemmArgs::ws_ld; +1/32 of the quantised weights' bytes).  A failed allocation only means the row-major scales stay in use.
    if (!c->f32 && c->layers.size() && !c->layers[0].sqkvT) {
        const lmrs_args& A = c->args;
        const bool tp = c->world > 1 || c->comm;
        const int dim = (int)A.dim, hid = (int)A.hidden_dim, att_full = tp && !c->cls_only ? c->att_full : c->att_dim;
        const int hid_l = tp && !c->cls_only ? c->hid_l : hid, dim_l = tp && !c->cls_only && !c->rep_out ? c->dim_l : dim;
        bool ok = true;
        auto tr = [&](const float* src, int rows, int groups) -> const float* {
            if (!ok) return nullptr;
            DevBuf<float> t;
            if (!t.alloc((size_t)rows * groups)) { (void)hipGetLastError(); ok = false; return nullptr; }
            float* d = t;
            c->scales_t.push_back(std::move(t));
            if (launch_transpose_scales(src, rows, groups, d, c->stream) != hipSuccess) { ok = false; return nullptr; }
            return d;
        };
        for (DevLayer& L : c->layers) {
            L.sqkvT = tr(L.sqkv, c->att_dim + 2 * c->kv_dim, dim / 128); L.soT = tr(L.so, dim_l, att_full / 128);
            L.s13T = tr(L.s13, 2 * hid_l, dim / 128); L.s2T = tr(L.s2, dim_l, hid / 128);
        }
        if (!ok) for (DevLayer& L : c->layers) L.sqkvT = L.soT = L.s13T = L.s2T = nullptr;
    }
    c->pf_ready = true;
    return 0;
}

// RoPE + attention of a batch (transformer.rs:443-544 inside the sl loop) on the rows the qkv GEMM left in pf_q / pf_k / the V cache.  Block attention
// (64-query blocks): the rotation rides in the score kernel's staging, which also writes the rotated keys to the cache (att_stage; round 6 - RoPE was a
// launch of its own).  Otherwise (a few tokens, or score slabs beyond 1 GiB): the RoPE launch, then one workgroup per (token, head).
// (the rule as a question of its own - lmrs_batch_prefill_form asks it without a pass: m rows of one sequence at p0 take block attention)
static bool prefill_block_route(const lmrs_ctx* c, int m, int p0) {
    AttnArgs t{};
    t.head_size = (int)c->args.head_size; t.n_heads = c->att_dim / t.head_size; t.n_kv_heads = c->kv_dim / t.head_size; t.gemma = c->args.model_type == LMRS_GEMMA;
    return attention_block_supported(t, m) && attention_block_scratch_floats(t.n_heads, m, p0 + m) <= ((size_t)1 << 28);    // <= 1 GiB of score slabs; longer contexts: per-token kernel
}
static int prefill_slabs(lmrs_ctx* c, size_t need) {                           // pf_att, grown to the pass's score slabs
    if (need <= c->pf_att.count()) return 0;
    if (c->pf_att) HIP_OK(hipStreamSynchronize(c->stream));
    return c->pf_att.alloc(need) ? 0 : alloc_failed("prefill score slabs: hipMalloc");
}
static int prefill_attention(lmrs_ctx* c, AttnArgs& t, int m, int p0) {
    if (prefill_block_route(c, m, p0)) {
        if (prefill_slabs(c, attention_block_scratch_floats(t.n_heads, m, p0 + m))) return -1;
        t.k_raw = c->pf_k;
        HIP_OK(launch_attention_block(t, p0, m, c->pf_att, c->sw.att_lds_keys, c->sw.att_long_batch_forms, c->stream));
        return 0;
    }
    HIP_OK(launch_rope_rows(c->pf_q, c->pf_k, t.k_cache, c->rope, t.n_heads, t.n_kv_heads, t.head_size, t.seq_len, t.layer, p0, m, c->stream));
    HIP_OK(launch_attention_rows(t, p0, m, c->stream));
    return 0;
}

// forward_layer(sl = m) for every layer over tokens at positions p0 .. p0+m-1 whose embeddings sit in c->pf_x.
// Gemma: the branch outputs go to pf_t and "x += rmsnorm(branch)" (transformer.rs:563-568, 643-650) is folded into the
// per-token prologue of the next GEMM (mode 2), as in the decode path; the last one is applied at the end.
// On ROW SHARDS (plan "tp"; prefill_tp_shapes_ok) every shard runs the GEMMs of its own rows over the token batch - its heads' q / k / v rows and
// attention, its gate / up pairs - and wo / w2 whole (replicated rows), so two exchanges per layer, as in the decode step: each shard quantises ITS
// slice of every token's att_out / h (whole 128-groups: bit for bit the groups of the gathered vector; Q4_0: the int8 (q - 8) octets the batched
// matmul_q4 reads), the blocks are all-gathered (RCCL, or the push transport's wide copy) and laid out as the next GEMM's activation operand.  The att
// and h blocks are TWO buffers: a peer can only write block A of layer l + 1 after it has seen this shard's flag of exchange H of layer l, which
// this shard raises after it has consumed A of layer l (stream order) - and the other way round.
static bool row_sharded(const lmrs_ctx* c);
static int prefill_layers(lmrs_ctx* c, PassForm form, int m, int p0) {
    const lmrs_args& a = c->args;
    const bool tp = row_sharded(c);
    const int dim = (int)a.dim, hid = (int)a.hidden_dim, att = c->att_dim, kv = c->kv_dim, hs = (int)a.head_size, q4 = c->q4, W = c->world;
    const int att_full = tp ? c->att_full : att, hid_l = tp ? c->hid_l : hid;
    const bool gemma = a.model_type == LMRS_GEMMA;
    const float eps = a.rms_norm_eps;
    float* const k_cache = form.k_cache ? form.k_cache : c->k_cache; float* const v_cache = form.v_cache ? form.v_cache : c->v_cache;
    float* const qkv = form.qkv ? form.qkv : c->pf_q;
    const bool table = form.rows || form.runs.tok;
    // scale layouts of this pass: from 48 tokens on every GEMM is a ring kernel, which takes TRANSPOSED scales ([group][row]: GemmArgs::ws_ld / xs_ld) -
    // the weights' transposed copies (prefill_alloc) and activation scales written that way by their producers, leading dimension kPrefillTokens
    // (the weight-streaming forms - PassForm::skinny, up to 64 rows - take row-major scales at any row count)
    const bool trs = m >= 48 && !form.skinny && c->layers[0].sqkvT != nullptr;
    const int xld = trs ? kPrefillTokens : 0;
    auto all_gather = [&](const float* mine, int n_l, char* blocks, size_t cap) -> int {          // mine: [m][n_l] f32 -> pf_xq / pf_xs [m][W * n_l]
        const size_t s_off = (size_t)m * n_l, bytes = s_off + (size_t)m * (n_l / 128) * 4, stride = pad256(bytes);
        if (stride > cap) return fail("prefill block overflow");
        char* blk = blocks + (size_t)c->rank * stride;
        HIP_OK(launch_quantize_rows(mine, n_l, m, q4, reinterpret_cast<int8_t*>(blk), reinterpret_cast<float*>(blk + s_off), c->stream));
        ExchangeDesc e{blocks, bytes, stride, nullptr, 0}; e.wide = true;
        if (enqueue_exchange(c, e)) return -1;
        HIP_OK(launch_gather_rows(blocks, stride, s_off, W, n_l, m, c->pf_xq, c->pf_xs, c->stream, xld));
        return 0;
    };
    // wo / w2 (g.wq, g.ws, g.n set by the caller): x += ... (Gemma: the branch buffer pf_t).  All rows on this shard, or - the split-out plan - its dim_l
    // rows into its block of pfx_x, an all-gather of the f32 slices, and the same single addition per element from the gathered blocks
    auto out_rows = [&](GemmArgs& g) -> int {
        float* dst = gemma ? c->pf_t : c->pf_x;
        if (!tp || c->rep_out) { g.o = dim; g.out = dst; if (trs) g.ws_ld = dim; HIP_OK(launch_gemm_q8(g, gemma ? EPI_STORE : EPI_RESID, c->stream)); return 0; }
        const size_t bytes = (size_t)m * c->dim_l * 4, stride = pad256(bytes);
        if (stride > c->pfb_x || !c->pfx_x) return fail("prefill block overflow");
        g.o = c->dim_l; g.out = reinterpret_cast<float*>(c->pfx_x + (size_t)c->rank * stride); if (trs) g.ws_ld = c->dim_l;
        HIP_OK(launch_gemm_q8(g, EPI_STORE, c->stream));
        ExchangeDesc e{c->pfx_x, bytes, stride, nullptr, 0}; e.wide = true;
        if (enqueue_exchange(c, e)) return -1;
        HIP_OK(launch_scatter_rows(c->pfx_x, stride, W, c->dim_l, m, dst, gemma ? 0 : 1, c->stream));
        return 0;
    };
    for (uint32_t l = 0; l < a.n_layers; ++l) {
        const DevLayer& L = c->layers[l];
        GemmArgs g{};
        g.xq = c->pf_xq; g.xs = c->pf_xs; g.n_tok = m; g.q4 = q4; g.xs_ld = xld; g.skinny = form.skinny;
        // [x += rmsnorm(previous ffn out)] rmsnorm + quantize | Wqkv | q, raw k, v rows -> cache      (transformer.rs:409-431)
        if (gemma && l > 0) HIP_OK(launch_rows_prologue(c->pf_x, L.rms_att, c->pf_t, c->layers[l - 1].rms_post_ffn, eps, 1, 2, q4, dim, m, c->pf_xq, c->pf_xs, c->stream, xld));
        else HIP_OK(launch_rows_prologue(c->pf_x, L.rms_att, nullptr, nullptr, eps, gemma, 1, q4, dim, m, c->pf_xq, c->pf_xs, c->stream, xld));
        g.wq = L.wqkv; g.ws = trs ? L.sqkvT : L.sqkv; g.ws_ld = trs ? att + 2 * kv : 0; g.n = dim; g.o = att + 2 * kv; g.out = qkv; g.k_raw = c->pf_k; g.v_cache = v_cache;
        g.att_dim = att; g.kv_dim = kv; g.seq_len = (int)a.seq_len; g.layer = (int)l; g.pos0 = p0;
        // (a row table: the rows' positions are not consecutive - q | raw k | v stay one [m][att + 2 kv] block in pf_q, plain stores as EPI_QKV's;
        // from 48 rows on the ring kernel writes it with the scales transposed as for EPI_QKV: ws_ld = the block's width, xs_ld = kPrefillTokens)
        HIP_OK(launch_gemm_q8(g, table ? EPI_STORE : EPI_QKV, c->stream));
        // RoPE, keys into the cache; attention (this shard's heads)                    (:443-544)
        AttnArgs t{};
        t.q = qkv; t.k_raw = nullptr; t.k_cache = k_cache; t.v_cache = v_cache; t.rope = c->rope; t.out = c->pf_ao;
        t.n_heads = att / hs; t.n_kv_heads = kv / hs; t.head_size = hs; t.seq_len = (int)a.seq_len; t.layer = (int)l;
        t.gemma = gemma; t.st = c->st;
        if (form.pages.tab) {
            // a paged batch: the table pass (either table, as a RowView) with every K / V address looked up in the slot's page row
            const RowView rv = form.rows ? RowView{form.rows->off, form.rows->pos, form.rows->tok} : form.runs;
            HIP_OK(launch_paged_scatter(qkv, k_cache, v_cache, c->rope, rv, form.pages, t.n_heads, t.n_kv_heads, hs, t.layer, m, c->stream));
            if (form.block_pos0 >= 0) {
                // one slot's consecutive rows, rotated and in its pages by now: 64-query blocks read every key and value row through the slot's page row
                if (prefill_slabs(c, attention_block_scratch_floats(t.n_heads, m, form.block_pos0 + m))) return -1;
                HIP_OK(launch_paged_attention_block(t, form.pages, form.block_row, form.block_pos0, m, c->pf_att, c->sw.att_lds_keys, c->sw.att_long_batch_forms, c->stream));
            } else HIP_OK(launch_paged_attention(t, rv, form.pages, m, form.max_T, c->stream));
        } else if (form.rows) {
            // every row at its own position in its own slot: rotation, K / V rows into the slots, one attention workgroup per (head, row)
            HIP_OK(launch_rope_scatter_rows(c->pf_q, k_cache, v_cache, c->rope, form.rows, t.n_heads, t.n_kv_heads, hs, t.seq_len, t.layer, m, c->stream));
            HIP_OK(launch_attention_table(t, form.rows, m, form.max_T, c->stream));
        } else if (form.runs.tok) {
            // the same over the long table: a row also sees the earlier rows of its own run, all stored before the attention launch starts
            HIP_OK(launch_rope_scatter_runs(qkv, k_cache, v_cache, c->rope, form.runs, t.n_heads, t.n_kv_heads, hs, t.seq_len, t.layer, m, c->stream));
            HIP_OK(launch_attention_runs(t, form.runs, m, form.max_T, c->stream));
        } else if (prefill_attention(c, t, m, p0)) return -1;
        // quantize | Wo | x += ... (Gemma: -> pf_t)                                     (:550-576)
        if (tp) { if (all_gather(c->pf_ao, att, c->pfx_att, c->pfb_att)) return -1; }
        else HIP_OK(launch_rows_prologue(c->pf_ao, nullptr, nullptr, nullptr, 0.f, 0, 0, q4, att, m, c->pf_xq, c->pf_xs, c->stream, xld));
        g.wq = L.wo; g.ws = trs ? L.soT : L.so; g.n = att_full;
        if (out_rows(g)) return -1;
        // [x += rmsnorm(attention out)] rmsnorm + quantize | W1, W3 | act(gate) * up  (:578-624)
        if (gemma) HIP_OK(launch_rows_prologue(c->pf_x, L.rms_pre_ffn, c->pf_t, L.rms_post_att, eps, 1, 2, q4, dim, m, c->pf_xq, c->pf_xs, c->stream, xld));
        else HIP_OK(launch_rows_prologue(c->pf_x, L.rms_post_att, nullptr, nullptr, eps, 0, 1, q4, dim, m, c->pf_xq, c->pf_xs, c->stream, xld));
        g.wq = L.w13; g.ws = trs ? L.s13T : L.s13; g.ws_ld = trs ? 2 * hid_l : 0; g.n = dim; g.o = 2 * hid_l; g.out = c->pf_h;
        // quantize | W2 | x += ... (Gemma: -> pf_t)                                     (:630-654)
        if (tp) {
            HIP_OK(launch_gemm_q8(g, gemma ? EPI_GELU : EPI_SWIGLU, c->stream));
            if (all_gather(c->pf_h, hid_l, c->pfx_h, c->pfb_h)) return -1;
        } else if (gemm_q8_hq_fused(dim, 2 * hid, m, q4 != 0)) {
            // (the quantiser of h in w1/w3's epilogue: int8 rows + scales in the buffer the f32 rows would have taken)
            g.hq = reinterpret_cast<int8_t*>(c->pf_h.get()); g.hs = reinterpret_cast<float*>(reinterpret_cast<char*>(c->pf_h.get()) + (size_t)kPrefillTokens * hid);
            g.hs_ld = xld;
            HIP_OK(launch_gemm_q8(g, gemma ? EPI_GELU_Q : EPI_SWIGLU_Q, c->stream));
            g.xq = g.hq; g.xs = g.hs;
        } else {
            HIP_OK(launch_gemm_q8(g, gemma ? EPI_GELU : EPI_SWIGLU, c->stream));
            HIP_OK(launch_rows_prologue(c->pf_h, nullptr, nullptr, nullptr, 0.f, 0, 0, q4, hid, m, c->pf_xq, c->pf_xs, c->stream, xld));
        }
        g.wq = L.w2; g.ws = trs ? L.s2T : L.s2; g.n = hid;
        if (out_rows(g)) return -1;
    }
    if (gemma) HIP_OK(launch_rows_addnorm(c->pf_x, c->pf_t, c->layers[a.n_layers - 1].rms_post_ffn, eps, dim, m, c->stream));
    return 0;
}
// (a communicator of ONE rank counts as a row-sharded context - the RCCL branch of the batched path can then run, and be tested, on a one-GPU box)
static bool row_sharded(const lmrs_ctx* c) { return (c->world > 1 || c->comm) && !c->cls_only; }
static bool prefill_tp_ok(const lmrs_ctx* c) { return c->tp_prefill && row_sharded(c) && (c->comm || (c->p2p && c->p2p_ready && c->pfx_att)); }
static int prefill_pass(lmrs_ctx* c, PassForm form, int m, int p0) {
    if (row_sharded(c)) c->ex_slot = 0;
    return prefill_layers(c, form, m, p0);
}

// forward_layer over rows p0 .. p0 + n - 1, kPrefillTokens at a time (a later chunk only needs the K/V rows of the earlier ones, exactly as inside
// the reference's single call): produce(i0, m) leaves the embedding rows of a chunk in pf_x, consume(i0, m) takes its finished residual rows from there
template <class Produce, class Consume> static int prefill_chunks(lmrs_ctx* c, PassForm form, uint32_t p0, size_t n, Produce produce, Consume consume) {
    for (size_t i0 = 0; i0 < n; i0 += kPrefillTokens) {
        const int m = (int)std::min<size_t>(kPrefillTokens, n - i0);
        if (produce(i0, m) || prefill_pass(c, form, m, (int)(p0 + i0)) || consume(i0, m)) return -1;
    }
    return 0;
}
// DevState::win_base of a pass over the positions from pos on (only Gemma-2's kernels read it).  One forward_layer(sl = n) call - fill_kv_cache, batched
// or token by token - tests the 4096-key window against its FIRST position for every token (the u32 `pos - t` of transformer.rs:525); a pass that
// stands for n Transformer::forward calls (the token entry points) tests every token against its OWN position: kWinPerQuery (lmrs_kernels.h)
static int pass_win_base(const lmrs_ctx* c, uint32_t pos, bool forward_calls) {
    return forward_calls && c->args.model_type == LMRS_GEMMA ? kWinPerQuery : (int)pos;
}

extern "C" int lmrs_fill_kv_cache(lmrs_ctx* c, float* embeddings, uint32_t n, uint32_t curr_pos, uint32_t* new_pos) {
    if (!c || !embeddings) return fail("NULL argument");
    if ((size_t)curr_pos + n > c->args.seq_len) return fail("positions out of range");
    HIP_OK(hipSetDevice(c->device));
    const size_t dim = c->args.dim;
    const bool tp_batched = n > 1 && prefill_tp_ok(c);
    // Row-sharded context without a batched pass: each token goes through the sharded layer segments (exchanges included), every shard ends with the
    // whole residual stream in x
    const bool by_segments = !c->g_layers && !tp_batched && !(c->cls_only && n > 1 && prefill_batched_ok(c));
    if (by_segments && !(c->comm || (c->p2p && c->p2p_ready))) return fail("fill_kv_cache: this sharded context has no transport (lock-step groups are driven by lmrs_group_forward)");
    const bool batched = !by_segments && (tp_batched || prefill_batched_ok(c)) && n > 1;
    if (batched) {
        // forward_layer(sl = n): GEMMs over the token batch on the int8 matrix cores
        if (prefill_alloc(c)) return -1;
        if (set_state(c, curr_pos, 0, pass_win_base(c, curr_pos, false))) return -1;
        auto upload_rows = [&](size_t i0, int m) -> int {
            HIP_OK(hipMemcpyAsync(c->pf_x, embeddings + i0 * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, c->stream));
            if (i0 == 0) HIP_OK(hipEventRecord(c->ev0, c->stream));                     // (measurement: the layers without the first upload / the last download)
            return 0;
        };
        auto download_rows = [&](size_t i0, int m) -> int {
            if (i0 + kPrefillTokens >= n) HIP_OK(hipEventRecord(c->ev1, c->stream));
            HIP_OK(hipMemcpyAsync(embeddings + i0 * dim, c->pf_x, (size_t)m * dim * 4, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        if (prefill_chunks(c, PassForm{}, curr_pos, n, upload_rows, download_rows)) return -1;
        if (set_state(c, curr_pos + n, 0)) return -1;
    } else {
        // forward_layer(sl = n) for every layer is, value for value, n single-token passes through the layers (causal; each token's arithmetic only
        // sees tokens <= itself): the layers-only graph of the decode step or, on row shards, the step's layer segments
        if (set_state(c, curr_pos, 0, pass_win_base(c, curr_pos, false))) return -1;
        for (uint32_t i = 0; i < n; ++i) {
            const StepForm f = step_form_for(c, curr_pos + i, /*merged=*/false);
            if (by_segments && split_scratch(c, f)) return -1;
            HIP_OK(hipMemcpyAsync(c->x, embeddings + (size_t)i * dim, dim * 4, hipMemcpyHostToDevice, c->stream));
            if (!by_segments) HIP_OK(hipGraphLaunch(c->g_layers, c->stream));
            else if (enqueue_step_sharded(c, f, /*layers_only=*/true)) return -1;
            HIP_OK(hipMemcpyAsync(embeddings + (size_t)i * dim, c->x, dim * 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (finish_call(c)) return -1;
    if (batched) { float ms = 0; if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->last_fill_ms = ms; }
    if (new_pos) *new_pos = curr_pos + n;
    return 0;
}

// ------------------------------------------------------------------ runs of token ids through the batched pass
// A run of n tokens whose logits nobody reads (a prompt: chat.rs:188-193) only has to leave its K/V rows behind.  n calls of Transformer::forward are
// forward_layer over the batch with three differences that only Gemma-2 shows: forward scales the embedding rows by sqrt(dim) (transformer.rs:326-332;
// fill_kv_cache takes its rows as given), every call tests the 4096-key window against its OWN position (one forward_layer(sl = n) call tests the
// first position for all: win_base, lmrs_kernels.h), and the logits' first `dim` columns are soft-capped (tokens_pass).
// Below a run length the decode steps are cheaper than the pass (its GEMMs run whole token tiles).  Llama / Phi: 8, the measured crossover of
// lmrs_generate_greedy's prompt (a 16-token pass of Llama-3.2-1B: 1.9 ms, about 4.5 decode steps).  Gemma-2: 8 as well, measured with
// tools/prompt_rate.py on Gemma-2-2B Q4_0 (profiles/prompt_rate_gemma2b_q4.txt): 4 tokens 4.04 ms batched against 3.37 ms of decode steps, 8
// tokens 4.01 against 6.71 ms - the smallest measured run at which the pass wins by more than the spread of three repetitions.
constexpr size_t kTokensBatchMin = 8, kTokensBatchMinGemma = 8;
static size_t tokens_batch_min(const lmrs_ctx* c) {
    if (c->sw.tokens_batch_min > 0) return (size_t)c->sw.tokens_batch_min;
    return c->args.model_type == LMRS_GEMMA ? kTokensBatchMinGemma : kTokensBatchMin;
}
static bool tokens_batched(const lmrs_ctx* c, size_t n) { return n >= tokens_batch_min(c) && (prefill_batched_ok(c) || prefill_tp_ok(c)); }

// The arguments every entry point that takes a run of token ids checks, in this order; `span`: the positions the call will touch from start_pos on
static int check_tokens(const lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, size_t span) {
    if (n == 0) return fail("no tokens given (n == 0)");
    if (!c || !tokens) return fail("NULL argument");
    if ((size_t)start_pos + span > c->args.seq_len) return fail("start_pos + " + std::to_string(span) + " positions exceeds seq_len");
    for (size_t i = 0; i < n; ++i) if (tokens[i] >= c->args.vocab_size) return fail("token " + std::to_string(i) + " out of range");
    return 0;
}
// The refusal of the entry points that have no sharded form; `what`: the subject of the sentence
static int refuse_sharded(const lmrs_ctx* c, const char* what) {
    if (c->world > 1 || c->comm || c->p2p)
        return fail(std::string(what) + " runs on single-GPU contexts only (lmrs_create); contexts of lmrs_create_sharded / lmrs_group_create are not supported");
    return 0;
}
static int upload_tokens(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos) {      // -> c->tokens[start_pos ..), through the pinned h_tok
    memcpy(c->h_tok, tokens, n * 4);
    HIP_OK(hipMemcpyAsync(c->tokens + start_pos, c->h_tok, n * 4, hipMemcpyHostToDevice, c->stream));
    return 0;
}
static int stage_tokens(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, size_t span) {
    if (check_tokens(c, tokens, n, start_pos, span)) return -1;
    HIP_OK(hipSetDevice(c->device));
    return upload_tokens(c, tokens, n, start_pos);
}
static int token_rows(lmrs_ctx* c, const uint32_t* tokens, int m) {        // embedding rows of the device tokens[0 .. m) -> pf_x, as forward builds them
    const float scale = c->args.model_type == LMRS_GEMMA ? sqrtf((float)c->args.dim) : 0.0f;
    HIP_OK(launch_dequant_rows(c->emb_q, c->emb_s, c->q4, tokens, m, (int)c->args.dim, c->pf_x, c->stream, scale));
    return 0;
}
// K/V rows start_pos .. start_pos + n - 1 from c->tokens; the caller sets the state that follows (the pass's own: only Gemma's kernels read one)
static int prefill_token_run(lmrs_ctx* c, uint32_t start_pos, size_t n) {
    if (prefill_alloc(c)) return -1;
    if (c->args.model_type == LMRS_GEMMA && set_state(c, start_pos, 0, pass_win_base(c, start_pos, true))) return -1;
    return prefill_chunks(c, PassForm{}, start_pos, n, [&](size_t i0, int m) { return token_rows(c, c->tokens + start_pos + i0, m); }, [](size_t, int) { return 0; });
}
// The decode step per token for n GIVEN tokens, already in c->tokens: prompt_end = start_pos + n makes every step embed the next given token instead
// of its own result (lmrs_generate_greedy's prompt phase); per_step(t) is enqueued behind step t, whose logits are in c->logits then
template <class PerStep> static int decode_given_tokens(lmrs_ctx* c, uint32_t start_pos, size_t n, PerStep per_step) {
    if (set_state(c, start_pos, start_pos + (uint32_t)n)) return -1;
    HIP_OK(launch_embed(embed_args(c), c->stream));
    for (size_t t = 0; t < n; ++t) if (launch_step(c, start_pos + (uint32_t)t) || per_step(t)) return -1;
    return 0;
}
// A run nobody reads the logits of: K/V rows start_pos .. start_pos + n - 1 from c->tokens and the state behind them - the batched pass from
// tokens_batch_min tokens on, else the decode steps (the classifier's result of every step goes nowhere)
static int fill_given_tokens(lmrs_ctx* c, uint32_t start_pos, size_t n) {
    if (!tokens_batched(c, n)) return decode_given_tokens(c, start_pos, n, [](size_t) { return 0; });
    return prefill_token_run(c, start_pos, n) || set_state(c, start_pos + (uint32_t)n, 0) ? -1 : 0;
}

extern "C" int lmrs_generate_greedy(lmrs_ctx* c, const uint32_t* prompt, size_t n_prompt, uint32_t n_new, uint32_t start_pos,
                                    uint32_t* out_tokens, double* seconds) {
    if (!c || !prompt || (!out_tokens && n_new)) return fail("NULL argument");
    const size_t steps = n_prompt + (n_new ? n_new - 1 : 0);
    if (stage_tokens(c, prompt, n_prompt, start_pos, steps)) return -1;
    HIP_OK(hipEventRecord(c->ev0, c->stream));
    // The reference feeds the prompt token by token and discards every logits vector but the last (chat.rs:188-193): all
    // prompt tokens except the last only have to leave their K/V rows behind, which is forward_layer over a batch - the
    // matrix-core path of fill_kv_cache, value for value what the per-token passes produce.
    size_t done = 0;
    if (tokens_batched(c, n_prompt - 1)) {
        if (prefill_token_run(c, start_pos, n_prompt - 1)) return -1;
        done = n_prompt - 1;
    }
    // (not decode_given_tokens: the steps run on past the prompt, several per graph launch where that is possible)
    if (set_state(c, start_pos + (uint32_t)done, start_pos + (uint32_t)n_prompt)) return -1;
    HIP_OK(launch_embed(embed_args(c), c->stream));
    const int K = c->multi_k;
    const bool multi = K > 1 && primary_graph(c) && !c->dbg && !c->sw.no_graph;
    for (size_t s = done; s < steps;) {
        const uint32_t p = start_pos + (uint32_t)s;
        const StepForm f = step_form_for(c, p), last = step_form_for(c, p + K - 1);
        // K steps in one launch while they fit the run and stay inside one form, below the split attention
        const bool k_steps = multi && s + K <= steps && !last.split_chunks && f.qa_mode == last.qa_mode;
        if (k_steps ? replay_steps(c, f, K) : launch_step(c, p)) return -1;
        s += k_steps ? K : 1;
    }
    HIP_OK(hipEventRecord(c->ev1, c->stream));
    if (n_new) HIP_OK(hipMemcpyAsync(c->h_tok, c->tokens + start_pos + n_prompt, (size_t)n_new * 4, hipMemcpyDeviceToHost, c->stream));
    if (finish_call(c)) return -1;
    if (n_new) memcpy(out_tokens, c->h_tok, (size_t)n_new * 4);
    if (seconds) { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, c->ev0, c->ev1)); *seconds = ms * 1e-3; }
    return 0;
}

// ------------------------------------------------------------------ scoring: the logits of every position of a token sequence
// (lmrs_forward_tokens) and the log-probability of each next token (lmrs_score_tokens); no reference counterpart - n calls of
// Transformer::forward (transformer.rs:316-384), value for value.

constexpr size_t kScoreBlockBytes = (size_t)512 << 20;     // the [tokens][vocab] logits block: at most 512 MiB (Llama-3.2-1B: 263 MB for 512 tokens)

// The batched path: forward_layer over the whole sequence (prefill_pass: the int8 matrix-core GEMMs), then the final rmsnorm + quantise of every
// token and the classifier as ONE GEMM over the token batch.  Both give what the decode step gives, bit for bit; Gemma-2 too, with
// what only forward calls do: embedding rows scaled by sqrt(dim) (token_rows), the window tested per query (pass_win_base), logits soft-capped.
// Not taken:
//   * a classifier whose written rows are not a multiple of 16 (launch_gemm_q8 runs whole 16-row tiles; e.g. a vocabulary of 4102);
//   * one token (that is one decode step) and everything prefill_batched_ok refuses (f32 files, other geometries, LMRS_NO_BATCHED_PREFILL=1).
// Those run the decode step token by token, as lmrs_generate_greedy feeds a prompt.
static bool score_batched_ok(const lmrs_ctx* c, size_t n) {
    return n > 1 && prefill_batched_ok(c) && cls_rows(c) % 16 == 0;
}

// rows whose reductions one call can hold: a token run is at most seq_len long, a ragged batch pass (lmrs_batch_forward_runs) kPrefillTokens rows of any positions
static size_t score_cap(const lmrs_ctx* c) { return std::max<size_t>(c->args.seq_len, kPrefillTokens); }

// one set of alloc_all's (whole or absent: any member speaks for it); `block`: the logits block too (forward_tokens and the batched path need it, token-by-token scoring does not)
static int score_alloc(lmrs_ctx* c, bool block) {
    const size_t V = c->args.vocab_size, T = score_cap(c), S = (size_t)score_chunks((int)V);
    const size_t rows = std::min<size_t>(kPrefillTokens, std::max<size_t>(1, kScoreBlockBytes / (V * 4)));
    if (!c->h_sc && !alloc_all({{c->sc_part, rows * S}, {c->sc_lp, T}, {c->sc_idx, T}, {c->h_sc, T * 12}})) {
        (void)hipGetLastError();
        return fail("scoring buffers: out of memory");
    }
    if (block && !c->sc_logits) {
        if (!c->sc_logits.alloc(rows * V)) {
            (void)hipGetLastError();
            return fail("scoring logits block (" + std::to_string(rows * V * 4 >> 20) + " MiB): out of memory");
        }
        c->sc_rows = (int)rows;
    }
    return 0;
}

// The k of the top-k entry points, checked before anything else (`vocab` 0: not known yet)
static int topk_check_k(uint32_t k, uint32_t vocab) {
    if (k == 0 || k > (uint32_t)kTopkMax) return fail("top-k: k = " + std::to_string(k) + " is outside 1 .. " + std::to_string(kTopkMax));
    if (vocab && k > vocab) return fail("top-k: k = " + std::to_string(k) + " exceeds vocab_size = " + std::to_string(vocab));
    return 0;
}

// alloc_all's, like score_alloc's; made anew when a call asks for more rows per launch or a larger k than the buffers hold
static int topk_alloc(lmrs_ctx* c, int rows, int k) {
    if (c->tk_rows && rows <= c->tk_rows && k <= c->tk_k) return 0;
    rows = std::max(rows, c->tk_rows); k = std::max(k, c->tk_k);
    c->tk_rows = c->tk_k = 0;
    const size_t T = score_cap(c), S = (size_t)score_chunks((int)c->args.vocab_size);
    if (!alloc_all({{c->tk_cand, (size_t)rows * S * k}, {c->tk_cnt, (size_t)rows * S}, {c->tk_idx, T * k}, {c->tk_val, T * k}, {c->tk_rank, T}, {c->h_tk, T * k * 8 + T * 4}})) {
        (void)hipGetLastError();
        return fail("top-k buffers: out of memory");
    }
    c->tk_rows = rows; c->tk_k = k;
    return 0;
}

// lmrs_score_tokens_topk's further results (k == 0: none are asked for)
struct TopkOut { uint32_t k; uint32_t* idx; float* logprob; uint32_t* rank; };

// The pinned h_sc in its two halves (score_alloc): score_cap doubles for the log-probabilities, then score_cap indices
struct HostScores { double* lp; uint32_t* idx; };
static HostScores host_scores(const lmrs_ctx* c) { return {reinterpret_cast<double*>(c->h_sc.get()), reinterpret_cast<uint32_t*>(c->h_sc + score_cap(c) * 8)}; }

// What becomes of the logits rows of a run of n tokens in c->tokens[start_pos ..).  out_logits != null: they go to the host as they are
// (lmrs_forward_tokens); else the reduction of every row - the next token's log-probability to c->sc_lp, sample_argmax to c->sc_idx - and with k the
// selection behind it (c->tk_idx / tk_val / tk_rank)
// targets: row r's next token (c->tokens) is the target of its log-probability; false: the rows are not a run (a row table) - sample_argmax only
// reduce_too: out_logits AND the reduction, both from the same slab (lmrs_batch_forward_runs)
struct RowSink { uint32_t start_pos; size_t n; float* out_logits; uint32_t k; bool targets = true; bool reduce_too = false; };

// rows r0 .. r0 + m - 1 of the run, ld columns written at row stride ld (the rest up to vocab_size is the classifier's zero tail)
static int reduce_rows(lmrs_ctx* c, const RowSink& to, const float* rows, int ld, int m, size_t r0) {
    const int V = (int)c->args.vocab_size;
    ScoreArgs s{rows, ld, ld, V, m, c->tokens + to.start_pos + r0 + 1, to.targets ? (int)std::max<long long>(0, (long long)to.n - 1 - (long long)r0) : 0,
                c->sc_part, c->sc_lp + r0, c->sc_idx + r0};
    HIP_OK(launch_score_rows(s, c->stream));
    if (!to.k) return 0;
    // the selection over the same rows, behind the reduction whose chunk summaries give the log-probabilities their m and sum
    TopkArgs t{rows, ld, ld, V, m, (int)to.k, s.tgt, s.n_tgt, c->sc_part, c->tk_cand, c->tk_cnt,
               c->tk_idx + r0 * to.k, c->tk_val + r0 * to.k, c->tk_rank + r0};
    HIP_OK(launch_topk_rows(t, c->stream));
    return 0;
}
static int copy_out_rows(lmrs_ctx* c, const RowSink& to, const float* rows, int ld, int m, size_t r0) {
    const int V = (int)c->args.vocab_size;
    float* dst = to.out_logits + r0 * (size_t)V;
    if (ld == V) { HIP_OK(hipMemcpyAsync(dst, rows, (size_t)m * V * 4, hipMemcpyDeviceToHost, c->stream)); return 0; }
    for (int r = 0; r < m; ++r) memset(dst + (size_t)r * V + ld, 0, (size_t)(V - ld) * 4);   // the unwritten tail [cls_rows, vocab)
    HIP_OK(hipMemcpy2DAsync(dst, (size_t)V * 4, rows, (size_t)ld * 4, (size_t)ld * 4, m, hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// The tail of a batched chunk behind its layers, rows i0 .. i0 + m - 1 of the run in x (pf_x, or the rows a ragged pass picked from it): final rmsnorm + quantise of every token
// (transformer.rs:341-343), row-major scales; the classifier over the batch (:345-372) in the pass's form, a slab of the logits block's sc_rows
// rows at a time; Gemma's soft-cap (:375-381); every slab to the sink
static int classify_rows(lmrs_ctx* c, PassForm form, const RowSink& to, float* x, size_t i0, int m) {
    const lmrs_args& a = c->args;
    const int dim = (int)a.dim, o = cls_rows(c);
    const bool gemma = a.model_type == LMRS_GEMMA;
    HIP_OK(launch_rows_prologue(x, c->rms_final, nullptr, nullptr, a.rms_norm_eps, gemma, 1, c->q4, dim, m, c->pf_xq, c->pf_xs, c->stream));
    for (int j0 = 0; j0 < m; j0 += c->sc_rows) {
        const int mj = std::min(c->sc_rows, m - j0);
        GemmArgs g{};
        g.wq = c->cls_q; g.ws = c->cls_s; g.xq = c->pf_xq + (size_t)j0 * dim; g.xs = c->pf_xs + (size_t)j0 * (dim / 128);
        g.n = dim; g.o = o; g.n_tok = mj; g.q4 = c->q4; g.out = c->sc_logits; g.skinny = form.skinny;
        HIP_OK(launch_gemm_q8(g, EPI_STORE, c->stream));
        if (gemma) HIP_OK(launch_softcap_rows(c->sc_logits, o, std::min(dim, o), mj, c->stream));
        // a batch's penalties (PassForm::penalties), in front of its masks: one launch a slab, and only for a slab that has a penalised row
        if (form.penalties.hist && std::any_of(form.penalties.h_of + i0 + j0, form.penalties.h_of + i0 + j0 + mj, [](const PenaltyRow& r) { return r.slot >= 0; }))
            HIP_OK(launch_penalty_rows(c->sc_logits, o, o, mj, form.penalties.hist, form.penalties.seq_len, form.penalties.pos, form.penalties.of + i0 + j0, form.penalties.max_n, c->stream));
        // a batch's masks (PassForm::masks): one launch a slab, and only for a slab that has a masked row
        if (form.masks.bits && std::any_of(form.masks.h_of + i0 + j0, form.masks.h_of + i0 + j0 + mj, [](int m) { return m >= 0; }))
            HIP_OK(launch_mask_rows(c->sc_logits, o, o, mj, form.masks.bits, form.masks.words, form.masks.of + i0 + j0, c->stream));
        // a batch's token automata (PassForm::autos): the same stores under the mask of the state each row's slot stands in, found on the device
        if (form.autos.of && std::any_of(form.autos.h_of + i0 + j0, form.autos.h_of + i0 + j0 + mj, [](const AutoRow& r) { return r.slot >= 0; }))
            HIP_OK(launch_auto_mask_rows(c->sc_logits, o, o, mj, form.autos.of + i0 + j0, form.autos.state, form.autos.words, c->stream));
        // a batch's candidate filters (PassForm::filters), behind everything that changes or clears a logit: one launch a slab, and only for a slab that has a filtered row
        if (form.filters.of && std::any_of(form.filters.h_of + i0 + j0, form.filters.h_of + i0 + j0 + mj, [](const FilterRow& r) { return r.slot >= 0; }))
            HIP_OK(launch_filter_rows(c->sc_logits, o, o, mj, form.filters.of + i0 + j0, c->stream));
        if (to.out_logits && copy_out_rows(c, to, c->sc_logits, o, mj, i0 + j0)) return -1;
        if ((!to.out_logits || to.reduce_too) && reduce_rows(c, to, c->sc_logits, o, mj, i0 + j0)) return -1;
    }
    return 0;
}

// The logits rows of a run to their sink; the tokens are in c->tokens and score_alloc / topk_alloc are done.  batched (score_batched_ok): the chain
// above, kPrefillTokens at a time, in the given form; else the decode step per token (the form says nothing there): same values
static int run_tokens(lmrs_ctx* c, const RowSink& to, PassForm form, bool batched) {
    const uint32_t start_pos = to.start_pos;
    const size_t n = to.n;
    if (batched) {
        if (prefill_alloc(c)) return -1;
        // (a row table: the positions live in the table and a call may enqueue many passes - its caller sets the one state, batch_state)
        if (!form.rows && set_state(c, start_pos, 0, pass_win_base(c, start_pos, true))) return -1;
        // (a row table: its token column is the run, n <= kRowTableMax rows - one chunk)
        if (prefill_chunks(c, form, start_pos, n, [&](size_t i0, int m) { return token_rows(c, form.rows ? form.rows->tok : c->tokens + start_pos + i0, m); },
                           [&](size_t i0, int m) { return classify_rows(c, form, to, c->pf_x, i0, m); })) return -1;
        return form.rows ? 0 : set_state(c, start_pos + (uint32_t)n, 0);
    }
    const size_t V = c->args.vocab_size;
    size_t r0 = 0;                                       // first position held in the logits block (forward_tokens)
    return decode_given_tokens(c, start_pos, n, [&](size_t t) -> int {
        if (!to.out_logits) return reduce_rows(c, to, c->logits, (int)V, 1, t);
        HIP_OK(hipMemcpyAsync(c->sc_logits + (t - r0) * V, c->logits, V * 4, hipMemcpyDeviceToDevice, c->stream));
        if (t + 1 - r0 == (size_t)c->sc_rows || t + 1 == n) {
            if (copy_out_rows(c, to, c->sc_logits, (int)V, (int)(t + 1 - r0), r0)) return -1;
            r0 = t + 1;
        }
        return 0;
    });
}

// out_logits != null: lmrs_forward_tokens (n x vocab floats to the host); else lmrs_score_tokens' results, and with tk.k those of the top-k form
static int tokens_pass(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, float* out_logits, float* logprobs, uint32_t* argmax,
                       double* sum_logprob, const TopkOut& tk = TopkOut{0, nullptr, nullptr, nullptr}) {
    // (stage_tokens in its two halves: the refusal and the first-use allocations sit between the checks and the upload, where they always did)
    if (check_tokens(c, tokens, n, start_pos, n)) return -1;
    if (tk.k && topk_check_k(tk.k, c->args.vocab_size)) return -1;
    if (refuse_sharded(c, "scoring")) return -1;
    HIP_OK(hipSetDevice(c->device));
    const bool batched = score_batched_ok(c, n);
    if (score_alloc(c, batched || out_logits)) return -1;
    if (tk.k && topk_alloc(c, batched ? c->sc_rows : 1, (int)tk.k)) return -1;
    if (upload_tokens(c, tokens, n, start_pos)) return -1;
    if (run_tokens(c, RowSink{start_pos, n, out_logits, tk.k}, PassForm{}, batched)) return -1;
    const HostScores h = host_scores(c);
    if (!out_logits) {
        if (n > 1) HIP_OK(hipMemcpyAsync(h.lp, c->sc_lp, (n - 1) * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(h.idx, c->sc_idx, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    const size_t nk = n * tk.k;                                                             // h_tk: nk indices, nk log-probabilities, n - 1 ranks
    if (tk.k) {
        HIP_OK(hipMemcpyAsync(c->h_tk, c->tk_idx, nk * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemcpyAsync(c->h_tk + nk * 4, c->tk_val, nk * 4, hipMemcpyDeviceToHost, c->stream));
        if (tk.rank && n > 1) HIP_OK(hipMemcpyAsync(c->h_tk + nk * 8, c->tk_rank, (n - 1) * 4, hipMemcpyDeviceToHost, c->stream));
    }
    if (finish_call(c)) return -1;
    if (tk.k) {
        memcpy(tk.idx, c->h_tk, nk * 4); memcpy(tk.logprob, c->h_tk + nk * 4, nk * 4);
        if (tk.rank && n > 1) memcpy(tk.rank, c->h_tk + nk * 8, (n - 1) * 4);
    }
    if (!out_logits) {
        double sum = 0.0;
        for (size_t t = 0; t + 1 < n; ++t) { if (logprobs) logprobs[t] = (float)h.lp[t]; sum += h.lp[t]; }
        if (argmax) memcpy(argmax, h.idx, n * 4);
        if (sum_logprob) *sum_logprob = sum;
    }
    return 0;
}

extern "C" int lmrs_forward_tokens(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, float* logits) {
    if (!logits) return fail("NULL argument");
    return tokens_pass(c, tokens, n, start_pos, logits, nullptr, nullptr, nullptr);
}

extern "C" int lmrs_score_tokens(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, float* logprobs, uint32_t* argmax,
                                 double* sum_logprob) {
    return tokens_pass(c, tokens, n, start_pos, nullptr, logprobs, argmax, sum_logprob);
}

extern "C" int lmrs_score_tokens_topk(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, uint32_t k, float* logprobs, uint32_t* argmax,
                                      double* sum_logprob, uint32_t* topk_idx, float* topk_logprob, uint32_t* target_rank) {
    if (topk_check_k(k, 0)) return -1;
    if (!topk_idx || !topk_logprob) return fail("NULL argument");
    return tokens_pass(c, tokens, n, start_pos, nullptr, logprobs, argmax, sum_logprob, TopkOut{k, topk_idx, topk_logprob, target_rank});
}

// lmrs_forward with the selection behind the step instead of the copy of the logits: 2k words cross to the host
extern "C" int lmrs_forward_topk(lmrs_ctx* c, uint32_t token, uint32_t pos, uint32_t k, uint32_t* idx, float* logits_k) {
    if (topk_check_k(k, 0)) return -1;
    if (!c || !idx || !logits_k) return fail("NULL argument");
    if (topk_check_k(k, c->args.vocab_size)) return -1;
    if (refuse_sharded(c, "top-k")) return -1;
    if (token >= c->args.vocab_size || pos >= c->args.seq_len) return step_once(c, token, pos);          // (its message; nothing is enqueued)
    HIP_OK(hipSetDevice(c->device));
    if (topk_alloc(c, 1, (int)k)) return -1;
    if (step_once(c, token, pos)) return -1;
    const int V = (int)c->args.vocab_size;
    TopkArgs t{c->logits, V, V, V, 1, (int)k, nullptr, 0, nullptr, c->tk_cand, c->tk_cnt, c->tk_idx, c->tk_val, nullptr};
    HIP_OK(launch_topk_rows(t, c->stream));
    HIP_OK(hipMemcpyAsync(c->h_tk, c->tk_idx, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(c->h_tk + (size_t)k * 4, c->tk_val, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    if (finish_call(c)) return -1;
    memcpy(idx, c->h_tk, (size_t)k * 4); memcpy(logits_k, c->h_tk + (size_t)k * 4, (size_t)k * 4);
    return 0;
}

// ------------------------------------------------------------------ a prompt from token ids (no reference counterpart: the loop of chat.rs:188-193
// with every sampler result ignored)
extern "C" int lmrs_tokens_path(const lmrs_ctx* c, size_t n, int* batched) {
    if (!c || !batched) return fail("NULL argument");
    *batched = tokens_batched(c, n) ? 1 : 0;
    return 0;
}

extern "C" int lmrs_prefill_tokens(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, uint32_t* new_pos) {
    if (stage_tokens(c, tokens, n, start_pos, n)) return -1;
    if (fill_given_tokens(c, start_pos, n) || finish_call(c)) return -1;
    if (new_pos) *new_pos = start_pos + (uint32_t)n;
    return 0;
}

// ------------------------------------------------------------------ short runs in one weight pass: verifying drafted tokens, speculative greedy generate
// (no reference counterpart: n calls of Transformer::forward + sample_argmax, value for value)
constexpr size_t kShortPassMax = 16;           // one 16-token MFMA tile: the skinny GEMM's token axis (gemm_skinny_kernel)
// a batch pass's GEMMs stream the weights up to this many rows (gemm_stream_kernel above 16).  Measured (profiles/batch_wide_*.txt): against
// the direct kernels the stream kernel wins at 17 .. 47 rows on both models; from 48 rows on the ring kernels beat it (the kernel itself serves up to 64)
constexpr size_t kStreamPassMax = 47;

// tokens_pass's chain (run_tokens) for m <= 16 tokens already in c->tokens[start_pos ..), with the skinny form - every GEMM, the layers' and the
// classifier's: one pass over the weights - and the reduction as its sink: the per-position sample_argmax goes to c->sc_idx[0 .. m) on the device.
// Batched wherever score_batched_ok holds; the rest (f32 files, other geometries, LMRS_NO_BATCHED_PREFILL=1, classifier rows that are no multiple
// of 16) runs the decode step per token: same values.
static int short_pass(lmrs_ctx* c, uint32_t start_pos, size_t m) {
    const bool batched = score_batched_ok(c, m);
    if (score_alloc(c, batched)) return -1;
    return run_tokens(c, RowSink{start_pos, m, nullptr, 0}, PassForm{/*skinny=*/true}, batched);
}
// one verify pass over c->h_tok[0 .. n) at start_pos -> argmax (host, n entries), *n_accept; the arguments are checked by the caller
static int verify_run(lmrs_ctx* c, size_t n, uint32_t start_pos, uint32_t* argmax, uint32_t* n_accept) {
    HIP_OK(hipMemcpyAsync(c->tokens + start_pos, c->h_tok, n * 4, hipMemcpyHostToDevice, c->stream));
    if (short_pass(c, start_pos, n)) return -1;
    uint32_t* h_idx = host_scores(c).idx;
    HIP_OK(hipMemcpyAsync(h_idx, c->sc_idx, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (finish_call(c)) return -1;
    memcpy(argmax, h_idx, n * 4);
    uint32_t acc = 0;
    while (acc + 1 < n && c->h_tok[acc + 1] == argmax[acc]) ++acc;
    *n_accept = acc;
    return 0;
}

extern "C" int lmrs_verify_tokens(lmrs_ctx* c, const uint32_t* tokens, size_t n, uint32_t start_pos, uint32_t* argmax, uint32_t* n_accept) {
    if (check_tokens(c, tokens, n, start_pos, n)) return -1;
    if (!argmax || !n_accept) return fail("NULL argument");
    if (n < 2 || n > kShortPassMax) return fail("lmrs_verify_tokens: n = " + std::to_string(n) + " is outside 2 .. " + std::to_string(kShortPassMax));
    if (refuse_sharded(c, "lmrs_verify_tokens")) return -1;
    HIP_OK(hipSetDevice(c->device));
    memcpy(c->h_tok, tokens, n * 4);
    return verify_run(c, n, start_pos, argmax, n_accept);
}

extern "C" int lmrs_generate_speculative(lmrs_ctx* c, const uint32_t* prompt, size_t n_prompt, uint32_t n_new, uint32_t start_pos,
                                         uint32_t max_draft, uint32_t ngram_max, uint32_t* out_tokens, uint32_t* stats4, double* seconds) {
    if (!c || !prompt || (!out_tokens && n_new)) return fail("NULL argument");
    const size_t steps = n_prompt + (n_new ? n_new - 1 : 0);
    if (check_tokens(c, prompt, n_prompt, start_pos, steps)) return -1;
    if (max_draft < 1 || max_draft >= kShortPassMax) return fail("lmrs_generate_speculative: max_draft = " + std::to_string(max_draft) + " is outside 1 .. " + std::to_string(kShortPassMax - 1));
    if (ngram_max < 1) return fail("lmrs_generate_speculative: ngram_max must be at least 1");
    if (refuse_sharded(c, "lmrs_generate_speculative")) return -1;
    HIP_OK(hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t st[4] = {0, 0, 0, 0};
    // the prompt but its last token only leaves K/V rows behind, as in lmrs_generate_greedy (n_new == 0: the whole prompt, as there)
    const size_t n_fill = n_new ? n_prompt - 1 : n_prompt;
    if (n_fill) {
        if (upload_tokens(c, prompt, n_fill, start_pos) || fill_given_tokens(c, start_pos, n_fill) || finish_call(c)) return -1;
    }
    std::vector<uint32_t> hist(prompt, prompt + n_prompt);
    hist.reserve(n_prompt + n_new);
    uint32_t pos = start_pos + (uint32_t)n_prompt - 1, draft[kShortPassMax], am[kShortPassMax];
    for (uint32_t done = 0; done < n_new;) {
        // hist ends with the last confirmed token, which runs at `pos`; a pass of 1 + k tokens gives at most k + 1 new ones
        uint32_t k = 0;
        const uint32_t room = std::min<uint32_t>(max_draft, n_new - done - 1);
        if (room && lmrs_draft_lookup(hist.data(), hist.size(), ngram_max, room, draft, &k)) return -1;
        uint32_t got = 1;
        if (k) {
            uint32_t acc = 0;
            c->h_tok[0] = hist.back();
            memcpy(c->h_tok + 1, draft, (size_t)k * 4);
            if (verify_run(c, (size_t)k + 1, pos, am, &acc)) return -1;
            got = acc + 1; st[0] += 1; st[1] += k; st[2] += acc;
        } else {
            if (lmrs_forward_argmax(c, hist.back(), pos, am)) return -1;
            st[3] += 1;
        }
        for (uint32_t i = 0; i < got; ++i) { out_tokens[done + i] = am[i]; hist.push_back(am[i]); }
        done += got; pos += got;
    }
    if (stats4) memcpy(stats4, st, sizeof st);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}


// ------------------------------------------------------------------ multi-sequence decode: up to 16 sequences a step over the context's weights
// (no reference counterpart: per row Transformer::forward + sample_argmax on a cache of its own, value for value).  A batch is n_slots more K/V
// caches of the context's layout; a step is run_tokens' batched arm, skinny, with a row table (PassForm::rows) - the qkv rows stay in scratch, one
// launch rotates them and scatters K / V into the rows' slots, and attention_rows_kernel's workgroups take slot and position from the table.
static int debug_kv_row(lmrs_ctx* c, const float* k_cache, const float* v_cache, int which, uint32_t layer, uint32_t pos, float* out, uint32_t page_len = 0);   // (with lmrs_debug_kv below)
// the ragged pass's table (lmrs_batch_forward_runs): RowTable's columns for kRunRowsMax rows, and sel - the table rows whose outputs were asked for, in output order
constexpr uint32_t kWideBatchMax = 64;         // a wide batch's slots, rows and runs
// fewest rows of a paged batch's prompt chunk that take block attention.  Measured by turns against the table pass (tools/batch_rate.py
// --paged-prefill): at position 0, 16 / 32 / 64 rows by block attention take 1.9x / 1.45x / 1.02x the table pass's time on Llama-3.2-1B Q8_0 and 2.0x / 1.95x /
// 1.06x on Gemma-2-2B Q4_0 (up to 47 rows the table pass also runs the weight-streaming GEMMs), 80 rows are within the turns' spread of it on both, 96 rows 0.93x
// on Llama but 1.003x, just outside the spread, on Gemma; from 112 rows on both are faster outside the spread (0.90x / 0.96x)
constexpr uint32_t kPagedBlockMin = 112;
struct RunTable { unsigned long long off[kRunRowsMax]; int pos[kRunRowsMax]; uint32_t tok[kRunRowsMax]; uint32_t sel[kRunRowsMax]; };
// The buffers of a sampled call (sample_set_alloc; rows != 0: the set stands, for that many rows): the rows' sampler table and its pinned source,
// launch_sample_rows' scratch, the result blocks ([rows][vocab + 1] words: {token, n0}, then the candidates) and the pinned copy of their heads (head_words each)
struct SampleSet {
    DevBuf<SampleRow> tab; PinBuf<SampleRow> h_tab; DevBuf<float> scratch; DevBuf<unsigned long long> out; PinBuf<unsigned long long> h_heads;
    size_t rows = 0, head_words = 0;
};
struct lmrs_batch {
    lmrs_ctx* c = nullptr; uint32_t n_slots = 0;
    uint32_t width = kRowTableMax;                      // the most rows / runs a call takes: 16, or kWideBatchMax for lmrs_batch_create_wide's batches
    // Every buffer is an owner (lmrs_buf.h): `delete b` frees them; the sets made after create are alloc_all's - whole or absent, their size word says which
    DevBuf<float> kv; size_t slot_floats = 0;           // [n_slots][K cache | V cache], slot_floats floats each: one allocation
    DevBuf<RowTable> tab; PinBuf<RowTable> h_tab;       // the pass's row table and its pinned source
    DevBuf<uint32_t> tokens;                            // a prefill's token run (seq_len)
    DevBuf<uint32_t> out; PinBuf<uint32_t> h_out;       // generate_greedy: [n_new][n] results of the passes, and their pinned copy (seq_len x 16)
    DevBuf<RunTable> runs; PinBuf<RunTable> h_runs;     // forward_runs: the long table and its pinned source,
    DevBuf<float> runs_qkv, runs_x;                     // its [kRunRowsMax][att + 2 kv] qkv block and the [kRunRowsMax][dim] rows picked for the classifier
    // forward_sample's set (kRowTableMax rows, made at the first call with a sampled row) and forward_runs_sample's own (whole sixteens up to the batch's width,
    // made anew when a call needs more), and the flat rows' keys / sorted pairs of the ragged call with their pinned copy (cs_words words)
    SampleSet samp, rs;
    DevBuf<unsigned long long> cs_keys; PinBuf<unsigned long long> h_cs_pairs; size_t cs_words = 0;
    DevBuf<float> embed_stage;                          // the embedding rows of a ragged pass, [kRunRowsMax][dim] in caller order (allocated at the first call that has one)
    // a paged batch (lmrs_batch_create_paged): kv is the pool - page p's K block at kv + p * 2 * page_floats, its V block page_floats behind, page 0 the zero
    // page; the accounting (lmrs_pages.h), the device page table [n_slots][per_slot] and its pinned mirror
    std::unique_ptr<PagePool> pool; uint32_t page_len = 0; size_t page_floats = 0;
    DevBuf<uint32_t> ptab; PinBuf<uint32_t> h_ptab;
    bool pf_table = false;                              // lmrs_batch_debug_prefill_table: every prompt chunk takes the table pass
    // allowed-token masks (lmrs_batch_set_masks; made at the first call, mask_words != 0 from then on): the device block [n_slots][mask_words] and its pinned mirror,
    // which is also the upload's staging; n_allowed[s] = 0: slot s has no mask, n_masked = the slots that have one.  mask_of / h_mask_of: the per-call
    // column of PassForm::masks, written with the tables (batch_rows, runs_table); mask_live: this call uploaded it - some output row of the call is masked
    DevBuf<uint32_t> masks; PinBuf<uint32_t> h_masks; size_t mask_words = 0;
    uint32_t n_allowed[kWideBatchMax] = {}; uint32_t n_masked = 0;
    DevBuf<int> mask_of; PinBuf<int> h_mask_of; bool mask_live = false;
    int mask_row_of(uint32_t slot) const { return n_allowed[slot] ? (int)slot : -1; }
    MaskView mask_view() const { return mask_live ? MaskView{masks, (int)mask_words, mask_of, h_mask_of} : MaskView{}; }
    // token automata (lmrs_batch_automaton_create / lmrs_batch_attach_automaton): the batch's automata, each with its tables on the host (the walks) and on
    // the device (class_of, next with the final flag in bit 31, the per-state masks the device built).  aut_of[s]: the automaton of slot s (-1: none), aut_q[s]
    // its state as the host knows it, n_aut the slots that have one.  aut_state: the state words on the device (made at the first attach, with the columns);
    // aut_dirty: the host moved a state since the last upload - the next call with such an output row uploads the words first; inside the device loops
    // gen_advance_kernel moves them and the host catches up by walking the reported tokens.  aut_rows / h_aut_rows: the per-call column of PassForm::autos,
    // written with the tables; aut_live: this call uploaded it
    struct Automaton {
        uint32_t n_states = 0, n_classes = 0, attached = 0;
        std::vector<uint16_t> class_of; std::vector<uint32_t> next, n_allowed; std::vector<uint8_t> final;
        DevBuf<uint16_t> d_class_of; DevBuf<uint32_t> d_next, d_masks;
        AutomatonTables tables(uint32_t V) const { return AutomatonTables{V, n_states, n_classes, class_of.data(), next.data(), final.data()}; }
    };
    std::unique_ptr<Automaton> automata[LMRS_AUTOMATA_MAX];
    int aut_of[kWideBatchMax]; uint32_t aut_q[kWideBatchMax] = {}; uint32_t n_aut = 0;
    DevBuf<uint32_t> aut_state; PinBuf<uint32_t> h_aut_state; bool aut_dirty = false;
    DevBuf<AutoRow> aut_rows; PinBuf<AutoRow> h_aut_rows; bool aut_live = false;
    lmrs_batch() { std::fill(aut_of, aut_of + kWideBatchMax, -1); }
    const Automaton* automaton_of(uint32_t slot) const { return aut_of[slot] >= 0 ? automata[aut_of[slot]].get() : nullptr; }
    AutoRow auto_row_of(uint32_t slot) const {
        const Automaton* a = automaton_of(slot);
        return a ? AutoRow{a->d_masks, a->d_class_of, a->d_next, a->n_classes, a->n_states, c->args.vocab_size, (int)slot} : AutoRow{nullptr, nullptr, nullptr, 0, 0, 0, -1};
    }
    AutoView auto_view() const { return aut_live ? AutoView{aut_rows, h_aut_rows, aut_state, (int)((c->args.vocab_size + 31) / 32)} : AutoView{}; }
    // the tokens slot's rows may produce now: its mask's count, or its automaton's current state's; 0: neither
    uint32_t allowed_now(uint32_t slot) const { const Automaton* a = automaton_of(slot); return a ? a->n_allowed[aut_q[slot]] : n_allowed[slot]; }
    // a slot standing in a final state that allows no token: no pass may ask for an output row of it
    bool auto_exhausted(uint32_t slot) const { const Automaton* a = automaton_of(slot); return a && !a->n_allowed[aut_q[slot]]; }
    // the token record and the penalties over it (lmrs_batch_set_history / lmrs_batch_set_penalties; made at the first call of either, `hist` non-null from then
    // on): hist[n_slots][seq_len], LMRS_TOKEN_NONE where the token is unknown.  hist_slot / h_hist_slot: the slot of every row of the pass's table, beside the
    // table (record_enqueue).  pen[s]: slot s's parameters, pen_on[s] - they are other than (1, 0, 0), n_pen the slots where they are.  pen_of / h_pen_of: the
    // per-call column of PassForm::penalties, written with the tables; pen_live: this call uploaded it - some output row of the call is penalised
    DevBuf<uint32_t> hist; DevBuf<int> hist_slot; PinBuf<int> h_hist_slot;
    struct Penalty { float repetition = 1.0f, presence = 0.0f, frequency = 0.0f; uint32_t out_from = 0; };
    Penalty pen[kWideBatchMax]; bool pen_on[kWideBatchMax] = {}; uint32_t n_pen = 0;
    DevBuf<PenaltyRow> pen_of; PinBuf<PenaltyRow> h_pen_of; bool pen_live = false;
    // candidate filters (lmrs_batch_set_filters; flt_of made at the first call that switches one on): flt[s] slot s's parameters as set, flt_on[s] - they can clear
    // a logit (0 < top_k < vocab_size, or a finite min_gap), n_flt the slots where they can.  flt_of / h_flt_of: the per-call column of PassForm::filters, written
    // with the tables; flt_live: this call uploaded it - some output row of the call is filtered
    struct Filter { uint32_t top_k = 0; float min_gap = INFINITY; };
    Filter flt[kWideBatchMax]; bool flt_on[kWideBatchMax] = {}; uint32_t n_flt = 0;
    DevBuf<FilterRow> flt_of; PinBuf<FilterRow> h_flt_of; bool flt_live = false;
    FilterRow filter_row_of(uint32_t slot) const { return flt_on[slot] ? FilterRow{(int)slot, flt[slot].top_k, flt[slot].min_gap} : FilterRow{-1, 0u, INFINITY}; }
    FilterView filter_view() const { return flt_live ? FilterView{flt_of, h_flt_of} : FilterView{}; }
    // lmrs_batch_generate (made at its first call; gen_st non-null: the set stands): the rows' state blocks beside the pass's table and their pinned mirror, the
    // live-row count and its pinned copy; `out` / `h_out` take the tokens [n][M].  gen_lp / h_gen_lp: the log-probabilities' block of the same layout (made at
    // the first call that asks for them, n * M words, made anew when a call needs more).  gen: the call's own sampling set (whole sixteens, as rs); gen_logits: the copy of the logits block the samplers
    // work on when a call wants log-probabilities too (gen_logits_rows rows)
    DevBuf<GenRow> gen_st; PinBuf<GenRow> h_gen_st; DevBuf<uint32_t> gen_live; PinBuf<uint32_t> h_gen_live;
    DevBuf<float> gen_lp; PinBuf<float> h_gen_lp;
    SampleSet gen; DevBuf<float> gen_logits; size_t gen_logits_rows = 0;
    // lmrs_batch_generate_topp (made at the first call with a top-p row, topp_vecs vectors; a call with more makes the set anew): per vector two blocks of
    // vocab_size pairs (ping-pong) and the sort's keys, the word that says which block holds it now (and its pinned copy), and topp_of / h_topp_of - the
    // column beside the pass's table that names every output row's vector by its number among the call's top-p rows, so no vector moves at a rebuild
    // topp_ext: per vector {from where its two blocks agree, how far the call has changed it}; h_topp: the vectors' pinned copies, upload source and download target
    DevBuf<unsigned long long> topp_state, topp_keys; DevBuf<uint32_t> topp_which, topp_ext, topp_of; PinBuf<uint32_t> h_topp_which, h_topp_ext, h_topp_of;
    PinBuf<unsigned long long> h_topp; size_t topp_vecs = 0;
    uint32_t* hist_of(uint32_t slot) const { return hist + (size_t)slot * c->args.seq_len; }
    PenaltyRow penalty_row_of(uint32_t slot, int tab_row) const {
        const Penalty& p = pen[slot];
        return pen_on[slot] ? PenaltyRow{(int)slot, tab_row, p.repetition, p.presence, p.frequency, p.out_from} : PenaltyRow{-1, 0, 1.0f, 0.0f, 0.0f, 0};
    }
    // table: the position column the rows' tab_row counts in (the row table's, or the long table's); max_n: the deepest row's position + 1 at this pass
    PenaltyView penalty_view(const int* table_pos, int max_n) const {
        return pen_live ? PenaltyView{hist, (int)c->args.seq_len, table_pos, pen_of, h_pen_of, max_n} : PenaltyView{};
    }
    RowView runs_view() const { return RowView{runs->off, runs->pos, runs->tok}; }      // (addresses inside the device table: nothing is read here)
    // the `off` word of a row of `slot`: where its caches start, in floats - on a paged batch its row of the page table
    unsigned long long off_of(uint32_t slot) const { return pool ? slot : (unsigned long long)slot * 2 * slot_floats; }
    PageView page_view() const {
        if (!pool) return PageView{};
        int sh = 0; while ((1u << sh) < page_len) ++sh;
        return PageView{ptab, (int)pool->per_slot(), sh, 2 * page_floats};
    }
    float* page_k(uint32_t page) const { return kv + (size_t)page * 2 * page_floats; }
    float* page_v(uint32_t page) const { return kv + (size_t)page * 2 * page_floats + page_floats; }
    float* k_of(uint32_t slot) const { return slot == LMRS_BATCH_CTX ? c->k_cache : kv + (size_t)slot * 2 * slot_floats; }
    float* v_of(uint32_t slot) const { return slot == LMRS_BATCH_CTX ? c->v_cache : kv + (size_t)slot * 2 * slot_floats + slot_floats; }
};

extern "C" void lmrs_batch_destroy(lmrs_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->c->device);
    (void)hipStreamSynchronize(b->c->stream);
    delete b;
}

// lmrs_batch_create / lmrs_batch_create_wide: `name` opens every message, width is the batch's row and slot limit
// page_len > 0 (lmrs_batch_create_paged): the slots draw pages of page_len positions from one pool of n_pages pages (+ the zero page) instead of a cache each
static int batch_create(lmrs_ctx* c, uint32_t n_slots, lmrs_batch** out, const std::string& name, uint32_t width, uint32_t page_len = 0, uint32_t n_pages = 0) {
    if (!c || !out) return fail("NULL argument");
    *out = nullptr;
    if (n_slots < 1 || n_slots > width) return fail(name + ": n_slots = " + std::to_string(n_slots) + " is outside 1 .. " + std::to_string(width));
    const lmrs_args& a = c->args;
    // the refusals, one message each: there is no token-by-token form of a batch step (the decode graphs' cache pointers are baked at capture)
    if (c->world > 1 && !c->comm && !c->p2p) return fail(name + ": members of a lock-step shard group (lmrs_group_create) are not supported");
    if (c->world > 1 || c->comm || c->p2p) return fail(name + ": sharded contexts (lmrs_create_sharded) are not supported");
    if (c->f32) return fail(name + ": unquantised (f32) files have no batched pass");
    if (c->sw.no_batched_prefill) return fail(name + ": the batched pass is switched off (LMRS_NO_BATCHED_PREFILL=1)");
    if (!prefill_batched_ok(c)) return fail(name + ": the batched pass is not built for this model's geometry");
    if (cls_rows(c) % 16) return fail(name + ": " + std::to_string(cls_rows(c)) + " classifier rows are not a multiple of 16");
    if (!score_batched_ok(c, 2)) return fail(name + ": this context has no batched pass for short runs");
    HIP_OK(hipSetDevice(c->device));
    if (prefill_alloc(c) || score_alloc(c, true)) return -1;
    if (c->sc_rows < kRowTableMax) return fail(name + ": the logits block holds fewer than " + std::to_string(kRowTableMax) + " rows of this vocabulary");
    lmrs_batch* b = new lmrs_batch;
    b->c = c; b->n_slots = n_slots; b->width = width; b->slot_floats = (size_t)a.n_layers * a.seq_len * c->kv_dim;
    b->page_len = page_len; b->page_floats = (size_t)a.n_layers * page_len * c->kv_dim;
    const size_t bytes = page_len ? ((size_t)n_pages + 1) * 2 * b->page_floats * 4 : (size_t)n_slots * 2 * b->slot_floats * 4, T = a.seq_len;
    if (!b->kv.alloc(bytes / 4)) {                                                                       // all or nothing: one allocation
        (void)hipGetLastError(); lmrs_batch_destroy(b);
        if (page_len) return fail(name + ": " + std::to_string(bytes) + " bytes of K/V pages for " + std::to_string(n_pages) + " pages (and the zero page): out of memory");
        return fail(name + ": " + std::to_string(bytes) + " bytes of K/V caches for " + std::to_string(n_slots) + " slots: out of memory");
    }
    if (page_len) {
        const uint32_t per_slot = (a.seq_len + page_len - 1) / page_len;
        b->pool.reset(new PagePool(n_slots, per_slot, page_len, n_pages));
        if (!alloc_all({{b->ptab, (size_t)n_slots * per_slot}, {b->h_ptab, (size_t)n_slots * per_slot}})) { (void)hipGetLastError(); lmrs_batch_destroy(b); return fail(name + ": page table: out of memory"); }
        memset(b->h_ptab, 0, (size_t)n_slots * per_slot * 4);
    }
    if (!alloc_all({{b->tab, 1}, {b->tokens, T}, {b->out, T * width}, {b->h_tab, 1}, {b->h_out, T * width}, {b->runs, 1}, {b->h_runs, 1},
                    {b->runs_qkv, (size_t)kRunRowsMax * (c->att_dim + 2 * c->kv_dim)}, {b->runs_x, (size_t)kRunRowsMax * a.dim}})) {
        (void)hipGetLastError(); lmrs_batch_destroy(b); return fail(name + ": row table and result buffers: out of memory");
    }
    // (a paged batch: the zero page and the table - every entry names the zero page; a page is cleared when it is claimed)
    if (page_len && hipMemsetAsync(b->ptab, 0, (size_t)n_slots * b->pool->per_slot() * 4, c->stream) != hipSuccess) { lmrs_batch_destroy(b); return fail(name + ": clearing the page table failed"); }
    if (hipMemsetAsync(b->kv, 0, page_len ? 2 * b->page_floats * 4 : bytes, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { lmrs_batch_destroy(b); return fail(name + ": clearing the caches failed"); }
    *out = b;
    return 0;
}

extern "C" int lmrs_batch_create(lmrs_ctx* c, uint32_t n_slots, lmrs_batch** out) { return batch_create(c, n_slots, out, "lmrs_batch_create", kRowTableMax); }
extern "C" int lmrs_batch_create_wide(lmrs_ctx* c, uint32_t n_slots, lmrs_batch** out) { return batch_create(c, n_slots, out, "lmrs_batch_create_wide", kWideBatchMax); }
extern "C" int lmrs_batch_width(const lmrs_batch* b, uint32_t* width) {
    if (!b || !width) return fail("NULL argument");
    *width = b->width;
    return 0;
}

// A batch call that fails after it began to enqueue drains the stream before it returns: nothing queued may still read the pinned row table or the
// state slot that the next call rewrites (ctx and batch stay usable); the failure's message stands
static int batch_failed(lmrs_ctx* c) { (void)hipStreamSynchronize(c->stream); c->err_queued = false; return -1; }
// the closing frame of a batch call: its enqueue, drained where that failed, then finish_call
template <class F> static int batch_call(lmrs_ctx* c, F&& enqueue) { return enqueue() ? batch_failed(c) : finish_call(c); }
// the one DevState of a batch call (only Gemma's kernels read it: every row tests the window against its own position)
static int batch_state(lmrs_ctx* c) { return set_state(c, 0, 0, pass_win_base(c, 0, true)); }

// ------------------------------------------------------------------ allowed-token masks: state of a slot (extensions, no reference counterpart)
// While slot s has a mask, every output row of s in any batch call is Sampler::sample / sample_argmax / the top-k definition over the row's logits with the
// disallowed entries -inf: classify_rows' one launch (mask_rows_kernel) between the soft-cap and the sinks, for the slabs that have a masked row.  No
// arithmetic on an allowed logit changes; a batch with no mask set runs exactly the launches it ran before.
static int masks_alloc(lmrs_batch* b) {
    if (b->mask_words) return 0;
    const size_t W = ((size_t)b->c->args.vocab_size + 31) / 32, bytes = (size_t)b->n_slots * W * 4;
    if (!alloc_all({{b->masks, bytes / 4}, {b->h_masks, bytes / 4}, {b->mask_of, kRunRowsMax}, {b->h_mask_of, kRunRowsMax}})) {
        (void)hipGetLastError();
        return fail("lmrs_batch_set_masks: " + std::to_string(bytes) + " bytes of masks for " + std::to_string(b->n_slots) + " slots (and as many pinned): out of memory");
    }
    memset(b->h_masks, 0, bytes);
    b->mask_words = W;
    return 0;
}
// the slots of a mask call, checked: `what` opens every message
static int mask_slots_check(const lmrs_batch* b, const std::string& what, uint32_t n, const uint32_t* slot, const char* noun = "mask ") {
    if (n > b->width) return fail(what + "n = " + std::to_string(n) + " exceeds the batch's width of " + std::to_string(b->width));
    uint64_t seen = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (slot[i] >= b->n_slots) return fail(what + noun + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " of " + std::to_string(b->n_slots));
        if (seen >> slot[i] & 1u) return fail(what + "slot " + std::to_string(slot[i]) + " appears twice");
        seen |= uint64_t(1) << slot[i];
    }
    return 0;
}
extern "C" int lmrs_batch_set_masks(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* bits) {
    const std::string what = "lmrs_batch_set_masks: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && (!slot || !bits)) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot)) return -1;
    lmrs_ctx* c = b->c;
    const size_t V = c->args.vocab_size, W = (V + 31) / 32;
    if (cls_rows(c) != (int)V) return fail(what + "the classifier leaves the last vocab_size % 4 logits unwritten: no masks for this vocabulary");
    for (uint32_t i = 0; i < n; ++i)
        if (b->aut_of[slot[i]] >= 0) return fail(what + "mask " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " has an automaton: one mask source per slot (a ban-list belongs in the automaton's classes)");
    const uint32_t last = V % 32 ? (1u << V % 32) - 1u : ~0u;                  // the bits of the last word that lie below vocab_size
    uint32_t count[kWideBatchMax];
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t* w = bits + (size_t)i * W;
        count[i] = (uint32_t)__builtin_popcount(w[W - 1] & last);
        for (size_t j = 0; j + 1 < W; ++j) count[i] += (uint32_t)__builtin_popcount(w[j]);
        if (!count[i]) return fail(what + "mask " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " would have no allowed token below vocab_size = " + std::to_string(V));
    }
    if (!n) return 0;
    HIP_OK(hipSetDevice(c->device));
    if (masks_alloc(b)) return -1;
    // the mirror's rows, then ONE copy: the span of rows from the lowest slot of the call to the highest (the rows between them go as they stand on the device)
    uint32_t lo = slot[0], hi = slot[0];
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(b->h_masks + (size_t)slot[i] * W, bits + (size_t)i * W, W * 4);
        b->h_masks[(size_t)slot[i] * W + W - 1] &= last;
        lo = std::min(lo, slot[i]); hi = std::max(hi, slot[i]);
    }
    if (hipMemcpyAsync(b->masks + (size_t)lo * W, b->h_masks + (size_t)lo * W, (size_t)(hi - lo + 1) * W * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        // (the slots of the call lose their masks: what the device holds for them is unknown)
        for (uint32_t i = 0; i < n; ++i) if (b->n_allowed[slot[i]]) { b->n_allowed[slot[i]] = 0; --b->n_masked; }
        return fail(what + std::string("uploading the masks failed: ") + hipGetErrorString(hipGetLastError()));
    }
    for (uint32_t i = 0; i < n; ++i) { if (!b->n_allowed[slot[i]]) ++b->n_masked; b->n_allowed[slot[i]] = count[i]; }
    return 0;
}
extern "C" int lmrs_batch_clear_masks(lmrs_batch* b, uint32_t n, const uint32_t* slot) {
    const std::string what = "lmrs_batch_clear_masks: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && !slot) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot)) return -1;
    if (!n) { memset(b->n_allowed, 0, sizeof b->n_allowed); b->n_masked = 0; return 0; }
    for (uint32_t i = 0; i < n; ++i) if (b->n_allowed[slot[i]]) { b->n_allowed[slot[i]] = 0; --b->n_masked; }
    return 0;
}
extern "C" int lmrs_batch_mask_info(const lmrs_batch* b, uint32_t slot, uint32_t* n_allowed) {
    const std::string what = "lmrs_batch_mask_info: ";
    if (!b || !n_allowed) return fail(what + "NULL argument");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    *n_allowed = b->allowed_now(slot);      // (a slot with an automaton: its current state's count)
    return 0;
}

// ------------------------------------------------------------------ token automata: a slot's mask follows the token it chose (extensions, no reference counterpart)
// A slot with an automaton has the mask of its current state: classify_rows' launch (auto_rows_mask_kernel) finds it through the slot's state word on the
// device, masks + state * W, so the device loops move a row's mask without the host (gen_advance_kernel stores the successor at the step boundary).  A batch
// that never attaches one enqueues exactly what it enqueued before: every hook tests b->n_aut.
static int automaton_index(const lmrs_batch* b, const lmrs_automaton* a) {
    for (int i = 0; i < LMRS_AUTOMATA_MAX; ++i) if (a && reinterpret_cast<const lmrs_automaton*>(b->automata[i].get()) == a) return i;
    return -1;
}
extern "C" int lmrs_batch_automaton_create(lmrs_batch* b, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next, const uint8_t* final,
                                           lmrs_automaton** out) {
    const char* name = "lmrs_batch_automaton_create";
    const std::string what = std::string(name) + ": ";
    if (!b || !out) return fail(what + "NULL argument");
    *out = nullptr;
    lmrs_ctx* c = b->c;
    const size_t V = c->args.vocab_size, W = (V + 31) / 32;
    if (cls_rows(c) != (int)V) return fail(what + "the classifier leaves the last vocab_size % 4 logits unwritten: no masks for this vocabulary");
    int at = 0;
    while (at < LMRS_AUTOMATA_MAX && b->automata[at]) ++at;
    if (at == LMRS_AUTOMATA_MAX) return fail(what + "the batch holds LMRS_AUTOMATA_MAX = " + std::to_string(LMRS_AUTOMATA_MAX) + " automata already");
    std::unique_ptr<lmrs_batch::Automaton> a;
    std::vector<uint32_t> coded;                         // next as the device holds it: the successor's final flag in bit 31
    try {
        a.reset(new lmrs_batch::Automaton);
        a->n_allowed.resize(n_states < kStateFinalBit ? n_states : 0u);             // (out of range: the check says so before it writes a count)
        if (automaton_check(name, AutomatonTables{(uint32_t)V, n_states, n_classes, class_of, next, final}, a->n_allowed.data(), false)) return -1;
        const size_t cells = (size_t)n_states * n_classes;
        a->n_states = n_states; a->n_classes = n_classes;
        a->class_of.assign(class_of, class_of + V); a->next.assign(next, next + cells);
        a->final.assign(n_states, 0);
        if (final) for (uint32_t q = 0; q < n_states; ++q) a->final[q] = final[q] ? 1 : 0;
        coded = a->next;
        for (uint32_t& e : coded) if (e != kAutoDead && a->final[e]) e |= kAutoFinalBit;
    } catch (...) { return fail(what + "out of memory on the host"); }                                  // nothing may unwind through the C ABI
    HIP_OK(hipSetDevice(c->device));
    const size_t cells = coded.size(), bytes = V * 2 + (cells + (size_t)n_states * W) * 4;
    if (!alloc_all({{a->d_class_of, V}, {a->d_next, cells}, {a->d_masks, (size_t)n_states * W}})) {
        (void)hipGetLastError();
        return fail(what + std::to_string(bytes) + " bytes of tables and masks for " + std::to_string(n_states) + " states: out of memory");
    }
    if (hipMemcpyAsync(a->d_class_of, a->class_of.data(), V * 2, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync(a->d_next, coded.data(), cells * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        launch_automaton_masks(a->d_class_of, a->d_next, (int)V, n_states, n_classes, a->d_masks, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(what + std::string("uploading the tables or building the masks failed: ") + hipGetErrorString(hipGetLastError()));
    b->automata[at] = std::move(a);
    *out = reinterpret_cast<lmrs_automaton*>(b->automata[at].get());
    return 0;
}
extern "C" int lmrs_batch_automaton_destroy(lmrs_batch* b, lmrs_automaton* a) {
    const std::string what = "lmrs_batch_automaton_destroy: ";
    if (!b || !a) return fail(what + "NULL argument");
    const int at = automaton_index(b, a);
    if (at < 0) return fail(what + "not an automaton of this batch");
    if (b->automata[at]->attached) return fail(what + std::to_string(b->automata[at]->attached) + " slots are attached to the automaton: detach them first");
    HIP_OK(hipSetDevice(b->c->device));
    HIP_OK(hipStreamSynchronize(b->c->stream));
    b->automata[at].reset();
    return 0;
}
extern "C" int lmrs_batch_attach_automaton(lmrs_batch* b, uint32_t n, const uint32_t* slot, lmrs_automaton* const* a, const uint32_t* state) {
    const std::string what = "lmrs_batch_attach_automaton: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && (!slot || !a)) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot, "row ")) return -1;
    int idx[kWideBatchMax];
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = what + "row " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + ": ";
        idx[i] = -1;
        if (!a[i]) continue;
        if (!state) return fail(what + "NULL array (state)");
        if ((idx[i] = automaton_index(b, a[i])) < 0) return fail(at + "not an automaton of this batch");
        const lmrs_batch::Automaton& A = *b->automata[idx[i]];
        if (b->n_allowed[slot[i]]) return fail(at + "the slot has a mask: one mask source per slot (clear it first; a ban-list belongs in the automaton's classes)");
        if (state[i] >= A.n_states) return fail(at + "start state " + std::to_string(state[i]) + " of " + std::to_string(A.n_states));
        if (!A.n_allowed[state[i]]) return fail(at + "start state " + std::to_string(state[i]) + " is final and allows no token");
    }
    if (!n) return 0;
    if (!b->aut_state) {
        HIP_OK(hipSetDevice(b->c->device));
        if (!alloc_all({{b->aut_state, kWideBatchMax}, {b->h_aut_state, kWideBatchMax}, {b->aut_rows, kRunRowsMax}, {b->h_aut_rows, kRunRowsMax}})) {
            (void)hipGetLastError();
            return fail(what + "state words and the passes' column: out of memory");
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = slot[i];
        if (b->aut_of[s] >= 0) { --b->automata[b->aut_of[s]]->attached; --b->n_aut; }
        b->aut_of[s] = idx[i]; b->aut_q[s] = idx[i] >= 0 ? state[i] : 0u;
        if (idx[i] >= 0) { ++b->automata[idx[i]]->attached; ++b->n_aut; }
    }
    b->aut_dirty = true;
    return 0;
}
extern "C" int lmrs_batch_automaton_state(const lmrs_batch* b, uint32_t slot, uint32_t* state, uint32_t* n_allowed, int* is_final) {
    const std::string what = "lmrs_batch_automaton_state: ";
    if (!b || !state) return fail(what + "NULL argument");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    const lmrs_batch::Automaton* a = b->automaton_of(slot);
    *state = a ? b->aut_q[slot] : LMRS_STATE_DEAD;
    if (n_allowed) *n_allowed = a ? a->n_allowed[b->aut_q[slot]] : 0u;
    if (is_final) *is_final = a ? (int)a->final[b->aut_q[slot]] : 0;
    return 0;
}
extern "C" int lmrs_batch_automaton_advance(lmrs_batch* b, uint32_t slot, const uint32_t* tokens, size_t n) {
    const char* name = "lmrs_batch_automaton_advance";
    const std::string what = std::string(name) + ": ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    const lmrs_batch::Automaton* a = b->automaton_of(slot);
    if (!a) return fail(what + "slot " + std::to_string(slot) + " has no automaton");
    uint32_t q = b->aut_q[slot]; size_t walked = 0;
    if (automaton_walk(name, a->tables(b->c->args.vocab_size), q, tokens, n, &q, &walked)) return -1;
    if (q != b->aut_q[slot]) { b->aut_q[slot] = q; b->aut_dirty = true; }
    return 0;
}

// ------------------------------------------------------------------ the token record and the penalties over it: state of a slot (extensions, no reference counterpart)
// hist[slot][pos] is the token whose K/V row stands at `pos` of `slot`: every batch call that writes K/V rows writes it too (record_rows_kernel over the pass's
// table, a copy for a contiguous prefill and a fork), so it is a function of the position - rewinds, rejected drafts, forks and releases need no bookkeeping,
// a row at position p reads hist[slot][0 .. p] only.  While slot s has penalties, every output row of s in any batch call is the row with
// penalty_rows_kernel's changes (lmrs_score.h: the rule, operation by operation), behind the soft-cap and in front of the slot's mask and every sink.
// A batch that made neither call enqueues exactly what it enqueued before: every hook below tests b->hist.
static_assert(LMRS_TOKEN_NONE == kTokenNone, "the header's NONE is the kernels'");
static int history_alloc(lmrs_batch* b, const std::string& what) {
    if (b->hist) return 0;
    const size_t words = (size_t)b->n_slots * b->c->args.seq_len;
    if (!alloc_all({{b->hist, words}, {b->hist_slot, kRunRowsMax}, {b->h_hist_slot, kRunRowsMax}, {b->pen_of, kRunRowsMax}, {b->h_pen_of, kRunRowsMax}})) {
        (void)hipGetLastError();
        return fail(what + std::to_string(words * 4) + " bytes of token record for " + std::to_string(b->n_slots) + " slots: out of memory");
    }
    if (hipMemsetAsync(b->hist, 0xFF, words * 4, b->c->stream) != hipSuccess || hipStreamSynchronize(b->c->stream) != hipSuccess) {
        b->hist.reset(); b->hist_slot.reset(); b->h_hist_slot.reset(); b->pen_of.reset(); b->h_pen_of.reset();
        return fail(what + std::string("clearing the token record failed: ") + hipGetErrorString(hipGetLastError()));
    }
    return 0;
}
extern "C" int lmrs_batch_set_history(lmrs_batch* b, uint32_t slot, uint32_t start_pos, const uint32_t* tokens, size_t n) {
    const std::string what = "lmrs_batch_set_history: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && !tokens) return fail(what + "NULL array");
    lmrs_ctx* c = b->c;
    const size_t V = c->args.vocab_size, T = c->args.seq_len;
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    if (start_pos > T || n > T - start_pos) return fail(what + "start_pos + n = " + std::to_string((size_t)start_pos + n) + " exceeds seq_len = " + std::to_string(T));
    for (size_t i = 0; i < n; ++i)
        if (tokens[i] >= V && tokens[i] != LMRS_TOKEN_NONE) return fail(what + "token " + std::to_string(i) + " out of range (neither below vocab_size = " + std::to_string(V) + " nor LMRS_TOKEN_NONE)");
    HIP_OK(hipSetDevice(c->device));
    if (history_alloc(b, what)) return -1;
    if (!n) return 0;
    if (hipMemcpyAsync(b->hist_of(slot) + start_pos, tokens, n * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(what + std::string("uploading the tokens failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}
extern "C" int lmrs_batch_history(lmrs_batch* b, uint32_t slot, uint32_t start_pos, size_t n, uint32_t* out) {
    const std::string what = "lmrs_batch_history: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && !out) return fail(what + "NULL array");
    lmrs_ctx* c = b->c;
    const size_t T = c->args.seq_len;
    if (!b->hist) return fail(what + "the batch keeps no token record (lmrs_batch_set_history or lmrs_batch_set_penalties switches it on)");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    if (start_pos > T || n > T - start_pos) return fail(what + "start_pos + n = " + std::to_string((size_t)start_pos + n) + " exceeds seq_len = " + std::to_string(T));
    if (!n) return 0;
    HIP_OK(hipSetDevice(c->device));
    if (hipMemcpyAsync(out, b->hist_of(slot) + start_pos, n * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(what + std::string("reading the record failed: ") + hipGetErrorString(hipGetLastError()));
    return 0;
}
extern "C" int lmrs_batch_set_penalties(lmrs_batch* b, uint32_t n, const uint32_t* slot, const float* repetition, const float* presence, const float* frequency,
                                        const uint32_t* out_from) {
    const std::string what = "lmrs_batch_set_penalties: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && (!slot || !repetition || !presence || !frequency || !out_from)) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot, "penalty ")) return -1;
    lmrs_ctx* c = b->c;
    const size_t V = c->args.vocab_size, T = c->args.seq_len;
    if (cls_rows(c) != (int)V) return fail(what + "the classifier leaves the last vocab_size % 4 logits unwritten: no penalties for this vocabulary");
    if (T > (size_t)kPenaltyKeysMax) return fail(what + "seq_len = " + std::to_string(T) + " exceeds the " + std::to_string(kPenaltyKeysMax) + " positions a penalised row sorts");
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = what + "penalty " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + ": ";
        if (!std::isfinite(repetition[i]) || !std::isfinite(presence[i]) || !std::isfinite(frequency[i])) return fail(at + "a value is not finite");
        if (!(repetition[i] > 0.0f)) return fail(at + "repetition = " + std::to_string(repetition[i]) + " is not above 0");
        if (out_from[i] > T) return fail(at + "out_from = " + std::to_string(out_from[i]) + " exceeds seq_len = " + std::to_string(T));
    }
    HIP_OK(hipSetDevice(c->device));
    if (history_alloc(b, what)) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = slot[i];
        const bool on = !(repetition[i] == 1.0f && presence[i] == 0.0f && frequency[i] == 0.0f);       // (1, 0, 0) changes no logit: the same as clearing
        b->pen[s] = lmrs_batch::Penalty{repetition[i], presence[i], frequency[i], out_from[i]};
        if (on && !b->pen_on[s]) ++b->n_pen;
        if (!on && b->pen_on[s]) --b->n_pen;
        b->pen_on[s] = on;
    }
    return 0;
}
extern "C" int lmrs_batch_clear_penalties(lmrs_batch* b, uint32_t n, const uint32_t* slot) {
    const std::string what = "lmrs_batch_clear_penalties: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && !slot) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot, "penalty ")) return -1;
    for (uint32_t s = 0; s < b->n_slots && !n; ++s) { b->pen[s] = lmrs_batch::Penalty{}; b->pen_on[s] = false; }
    if (!n) b->n_pen = 0;
    for (uint32_t i = 0; i < n; ++i) { if (b->pen_on[slot[i]]) --b->n_pen; b->pen[slot[i]] = lmrs_batch::Penalty{}; b->pen_on[slot[i]] = false; }
    return 0;
}
extern "C" int lmrs_batch_penalty_info(const lmrs_batch* b, uint32_t slot, float* repetition, float* presence, float* frequency, uint32_t* out_from, int* active) {
    const std::string what = "lmrs_batch_penalty_info: ";
    if (!b || !repetition || !presence || !frequency || !out_from || !active) return fail(what + "NULL argument");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    const lmrs_batch::Penalty& p = b->pen[slot];
    *repetition = p.repetition; *presence = p.presence; *frequency = p.frequency; *out_from = p.out_from; *active = b->pen_on[slot] ? 1 : 0;
    return 0;
}
// ------------------------------------------------------------------ candidate filters: top_k and min_gap, state of a slot (extensions, no reference counterpart)
// While slot s has a filter, every output row of s in any batch call but lmrs_batch_generate_greedy is the row with filter_rows_kernel's -inf stores
// (lmrs_score.h: the rule), behind the soft-cap, the penalties and the masks and in front of every sink.  A batch on which none was ever switched on has no
// column and enqueues exactly what it enqueued before: every hook tests b->n_flt.
static bool filter_active(const lmrs_batch* b, uint32_t top_k, float min_gap) { return (top_k != 0u && top_k < b->c->args.vocab_size) || min_gap < INFINITY; }
extern "C" int lmrs_batch_set_filters(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* top_k, const float* min_gap) {
    const std::string what = "lmrs_batch_set_filters: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && (!slot || !top_k || !min_gap)) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot, "filter ")) return -1;
    lmrs_ctx* c = b->c;
    if (cls_rows(c) != (int)c->args.vocab_size) return fail(what + "the classifier leaves the last vocab_size % 4 logits unwritten: no filters for this vocabulary");
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = what + "filter " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + ": ";
        if (min_gap[i] != min_gap[i]) return fail(at + "min_gap is NaN");
        if (min_gap[i] < 0.0f) return fail(at + "min_gap = " + std::to_string(min_gap[i]) + " is negative");
        any = any || filter_active(b, top_k[i], min_gap[i]);
    }
    if (any && !b->flt_of) {
        HIP_OK(hipSetDevice(c->device));
        if (!alloc_all({{b->flt_of, kRunRowsMax}, {b->h_flt_of, kRunRowsMax}})) {
            (void)hipGetLastError();
            return fail(what + "the filters' column: out of memory");
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = slot[i];
        const bool on = filter_active(b, top_k[i], min_gap[i]);            // (0, +inf) and top_k >= vocab_size clear no logit: the same as clearing
        b->flt[s] = lmrs_batch::Filter{top_k[i], min_gap[i]};
        if (on && !b->flt_on[s]) ++b->n_flt;
        if (!on && b->flt_on[s]) --b->n_flt;
        b->flt_on[s] = on;
    }
    return 0;
}
extern "C" int lmrs_batch_clear_filters(lmrs_batch* b, uint32_t n, const uint32_t* slot) {
    const std::string what = "lmrs_batch_clear_filters: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (n && !slot) return fail(what + "NULL array");
    if (mask_slots_check(b, what, n, slot, "filter ")) return -1;
    for (uint32_t s = 0; s < b->n_slots && !n; ++s) { b->flt[s] = lmrs_batch::Filter{}; b->flt_on[s] = false; }
    if (!n) b->n_flt = 0;
    for (uint32_t i = 0; i < n; ++i) { if (b->flt_on[slot[i]]) --b->n_flt; b->flt[slot[i]] = lmrs_batch::Filter{}; b->flt_on[slot[i]] = false; }
    return 0;
}
extern "C" int lmrs_batch_filter_info(const lmrs_batch* b, uint32_t slot, uint32_t* top_k, float* min_gap, int* active) {
    const std::string what = "lmrs_batch_filter_info: ";
    if (!b || !top_k || !min_gap || !active) return fail(what + "NULL argument");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    *top_k = b->flt[slot].top_k; *min_gap = b->flt[slot].min_gap; *active = b->flt_on[slot] ? 1 : 0;
    return 0;
}

// A fork's record: dst's first n_pos positions are src's; the context's sequence (LMRS_BATCH_CTX) has no record - unknown tokens
static int history_fork(lmrs_batch* b, uint32_t src_slot, uint32_t dst_slot, uint32_t n_pos) {
    if (!b->hist) return 0;
    if (src_slot == LMRS_BATCH_CTX) HIP_OK(hipMemsetAsync(b->hist_of(dst_slot), 0xFF, (size_t)n_pos * 4, b->c->stream));
    else HIP_OK(hipMemcpyAsync(b->hist_of(dst_slot), b->hist_of(src_slot), (size_t)n_pos * 4, hipMemcpyDeviceToDevice, b->c->stream));
    return 0;
}
// The record of a pass over the device table as it stands (its pos / tok columns; the slot column went up with the table, record_enqueue): R rows, one launch
static int record_rows(lmrs_batch* b, const int* pos, const uint32_t* tok, size_t R) {
    if (!b->hist) return 0;
    HIP_OK(launch_record_rows(b->hist, (int)b->c->args.seq_len, (int)b->n_slots, pos, tok, b->hist_slot, (int)R, b->c->stream));
    return 0;
}

// ------------------------------------------------------------------ paged batches: the slots draw pages from one pool (extensions, no reference counterpart)
// The accounting is lmrs_pages.cpp's, decided on the host and finished before any device work of the call; what it asks of the device - clear a
// claimed page, copy a page that is being un-shared, the table rows that changed - is enqueued here, in stream order ahead of the pass.
extern "C" int lmrs_batch_create_paged(lmrs_ctx* c, uint32_t n_slots, uint32_t page_len, uint32_t n_pages, lmrs_batch** out) {
    const std::string name = "lmrs_batch_create_paged";
    if (out) *out = nullptr;
    if (page_len != 64 && page_len != 128 && page_len != 256 && page_len != 512 && page_len != 1024)
        return fail(name + ": page_len = " + std::to_string(page_len) + " is none of 64, 128, 256, 512, 1024");
    if (n_pages == 0) return fail(name + ": n_pages is 0");
    return batch_create(c, n_slots, out, name, kWideBatchMax, page_len, n_pages);
}
extern "C" int lmrs_batch_pages(const lmrs_batch* b, uint32_t* page_len, uint32_t* n_pages, uint32_t* n_free) {
    if (!b || !page_len || !n_pages || !n_free) return fail("lmrs_batch_pages: NULL argument");
    if (!b->pool) return fail("lmrs_batch_pages: not a paged batch (lmrs_batch_create_paged)");
    *page_len = b->page_len; *n_pages = b->pool->n_pages(); *n_free = b->pool->n_free();
    return 0;
}
extern "C" int lmrs_batch_slot_pages(const lmrs_batch* b, uint32_t slot, uint32_t* n_held, uint32_t* n_shared) {
    if (!b || !n_held || !n_shared) return fail("lmrs_batch_slot_pages: NULL argument");
    if (!b->pool) return fail("lmrs_batch_slot_pages: not a paged batch (lmrs_batch_create_paged)");
    if (slot >= b->n_slots) return fail("lmrs_batch_slot_pages: slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    b->pool->slot_pages(slot, n_held, n_shared);
    return 0;
}
// the table rows of `dirty` slots: pinned mirror, then the device table (stream order; every batch call drains the stream before it returns, so the
// mirror is never rewritten under a copy in flight)
static int pages_upload(lmrs_batch* b, const std::vector<uint32_t>& dirty) {
    const size_t per = b->pool->per_slot();
    for (uint32_t s : dirty) {
        memcpy(b->h_ptab + s * per, b->pool->row(s), per * 4);
        HIP_OK(hipMemcpyAsync(b->ptab + s * per, b->h_ptab + s * per, per * 4, hipMemcpyHostToDevice, b->c->stream));
    }
    return 0;
}
static int pages_enqueue(lmrs_batch* b, const std::vector<PageAction>& acts, const std::vector<uint32_t>& dirty) {
    const size_t bytes = 2 * b->page_floats * 4;
    for (const PageAction& a : acts) {
        if (a.dst == 0 || a.dst > b->pool->n_pages() || a.src > b->pool->n_pages()) return fail("page accounting: an action outside the pool");
        if (a.kind == PageAction::kClear) HIP_OK(hipMemsetAsync(b->page_k(a.dst), 0, bytes, b->c->stream));
        else HIP_OK(hipMemcpyAsync(b->page_k(a.dst), b->page_k(a.src), bytes, hipMemcpyDeviceToDevice, b->c->stream));
    }
    return pages_upload(b, dirty);
}
// A call that writes the given ranges of a paged batch (no-op on any other): plan, commit, enqueue.  Short of pages the call fails here with nothing
// changed: `what` opens the message ("name: "), which gives the pages wanted and the pages free.
static int pages_claim(lmrs_batch* b, const std::string& what, const PageRange* ranges, size_t n) {
    if (!b->pool) return 0;
    std::vector<PageAction> acts; std::vector<uint32_t> dirty; uint32_t wanted = 0;
    if (!b->pool->write(ranges, n, &acts, &dirty, &wanted))
        return fail(what + std::to_string(wanted) + " pages wanted, " + std::to_string(b->pool->n_free()) + " free (the pool holds " + std::to_string(b->pool->n_pages()) + ")");
    if (acts.empty() && dirty.empty()) return 0;
    HIP_OK(hipSetDevice(b->c->device));
    if (pages_enqueue(b, acts, dirty)) return batch_failed(b->c);
    return 0;
}
// (the rows of a step: row i writes positions [pos[i], pos[i] + span) of slot[i]; the runs of a ragged pass)
static int pages_claim_rows(lmrs_batch* b, const std::string& what, uint32_t n, const uint32_t* slot, const uint32_t* pos, const uint32_t* len, uint32_t span) {
    if (!b->pool) return 0;
    std::vector<PageRange> r(n);
    for (uint32_t i = 0; i < n; ++i) r[i] = PageRange{slot[i], pos[i], pos[i] + (len ? len[i] : span)};
    return pages_claim(b, what, r.data(), n);
}
extern "C" int lmrs_batch_release(lmrs_batch* b, uint32_t slot, uint32_t n_pos) {
    if (!b) return fail("lmrs_batch_release: NULL argument");
    if (!b->pool) return fail("lmrs_batch_release: not a paged batch (lmrs_batch_create_paged)");
    if (slot >= b->n_slots) return fail("lmrs_batch_release: slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    if (n_pos > b->c->args.seq_len) return fail("lmrs_batch_release: n_pos = " + std::to_string(n_pos) + " exceeds seq_len");
    std::vector<uint32_t> dirty;
    b->pool->release(slot, n_pos, &dirty);
    if (dirty.empty()) return 0;
    HIP_OK(hipSetDevice(b->c->device));
    if (pages_upload(b, dirty)) return batch_failed(b->c);
    HIP_OK(hipStreamSynchronize(b->c->stream));
    return 0;
}
// lmrs_batch_prefill and lmrs_batch_prefill_embeddings on a paged batch: the table pass, one run per chunk of at most kRunRowsMax rows (defined
// with the ragged pass below)
static int paged_prefill(const std::string& what, lmrs_batch* b, uint32_t slot, const uint32_t* tokens, const float* embeddings, size_t n, uint32_t start_pos, float* residual);

extern "C" int lmrs_batch_prefill(lmrs_batch* b, uint32_t slot, const uint32_t* tokens, size_t n, uint32_t start_pos) {
    if (!b) return fail("NULL argument");
    lmrs_ctx* c = b->c;
    if (check_tokens(c, tokens, n, start_pos, n)) return -1;
    if (slot >= b->n_slots) return fail("lmrs_batch_prefill: slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    if (b->pool) return n ? paged_prefill("lmrs_batch_prefill: ", b, slot, tokens, nullptr, n, start_pos, nullptr) : 0;
    if (n == 1) {                                        // one token: lmrs_batch_forward's pass with nobody reading its result
        uint32_t am = 0;
        return lmrs_batch_forward(b, 1, &slot, tokens, &start_pos, &am, nullptr);
    }
    HIP_OK(hipSetDevice(c->device));
    memcpy(c->h_tok, tokens, n * 4);
    auto enqueue = [&]() -> int {
        HIP_OK(hipMemcpyAsync(b->tokens, c->h_tok, n * 4, hipMemcpyHostToDevice, c->stream));
        if (b->hist) HIP_OK(hipMemcpyAsync(b->hist_of(slot) + start_pos, b->tokens, n * 4, hipMemcpyDeviceToDevice, c->stream));     // the record: the run as it stands on the device
        if (batch_state(c)) return -1;
        PassForm form; form.skinny = n < kShortPassMax; form.k_cache = b->k_of(slot); form.v_cache = b->v_of(slot);
        return prefill_chunks(c, form, start_pos, n, [&](size_t i0, int m) { return token_rows(c, b->tokens + i0, m); }, [](size_t, int) { return 0; });
    };
    return batch_call(c, enqueue);
}

extern "C" int lmrs_batch_fork(lmrs_batch* b, uint32_t src_slot, uint32_t dst_slot, uint32_t n_pos) {
    if (!b) return fail("NULL argument");
    lmrs_ctx* c = b->c;
    const lmrs_args& a = c->args;
    if ((src_slot != LMRS_BATCH_CTX && src_slot >= b->n_slots) || dst_slot >= b->n_slots)
        return fail("lmrs_batch_fork: slots " + std::to_string(src_slot) + " -> " + std::to_string(dst_slot) + " of " + std::to_string(b->n_slots));
    if (src_slot == dst_slot) return fail("lmrs_batch_fork: source and destination are the same slot");
    if (n_pos > a.seq_len) return fail("lmrs_batch_fork: n_pos = " + std::to_string(n_pos) + " exceeds seq_len");
    if (n_pos == 0) return 0;
    HIP_OK(hipSetDevice(c->device));
    const size_t S = a.seq_len, kv = (size_t)c->kv_dim;
    if (b->pool) {
        // a paged batch: the whole pages become references, at most one page is copied; rows [r0, r1) of a page's K / V blocks from `ks` / `vs`, whose rows
        // lie ss positions apart (another page: page_len; the context's cache: seq_len)
        const size_t PL = b->page_len;
        auto copy_rows = [&](uint32_t page, size_t r0, size_t r1, const float* ks, const float* vs, size_t ss) -> int {
            HIP_OK(hipMemcpy2DAsync(b->page_k(page) + r0 * 4, PL * 16, ks, ss * 16, (r1 - r0) * 16, (size_t)a.n_layers * kv / 4, hipMemcpyDeviceToDevice, c->stream));
            HIP_OK(hipMemcpy2DAsync(b->page_v(page) + r0 * kv, PL * kv * 4, vs, ss * kv * 4, (r1 - r0) * kv * 4, a.n_layers, hipMemcpyDeviceToDevice, c->stream));
            return 0;
        };
        if (src_slot == LMRS_BATCH_CTX) {                // a contiguous source: its rows are copied into pages dst holds alone
            const PageRange all{dst_slot, 0, n_pos};
            if (pages_claim(b, "lmrs_batch_fork: ", &all, 1)) return -1;
            for (size_t p0 = 0; p0 < n_pos; p0 += PL) {
                const size_t p1 = std::min<size_t>(n_pos, p0 + PL);
                if (copy_rows(b->pool->row(dst_slot)[p0 / PL], 0, p1 - p0, c->k_cache + p0 * 4, c->v_cache + p0 * kv, S)) return batch_failed(c);
            }
        } else {
            std::vector<PageAction> acts; std::vector<uint32_t> dirty; uint32_t wanted = 0, part_p0 = 0, part_src = 0, part_dst = 0;
            if (!b->pool->fork(src_slot, dst_slot, n_pos, &acts, &dirty, &wanted, &part_p0, &part_src, &part_dst))
                return fail("lmrs_batch_fork: " + std::to_string(wanted) + " pages wanted, " + std::to_string(b->pool->n_free()) + " free (the pool holds " + std::to_string(b->pool->n_pages()) + ")");
            if (pages_enqueue(b, acts, dirty)) return batch_failed(c);
            if (part_dst && copy_rows(part_dst, 0, n_pos - part_p0, b->page_k(part_src), b->page_v(part_src), PL)) return batch_failed(c);
        }
        if (history_fork(b, src_slot, dst_slot, n_pos)) return batch_failed(c);
        HIP_OK(hipStreamSynchronize(c->stream));
        return 0;
    }
    // K: [layer][kv head][head / 4] pieces of S x 4 floats, the first n_pos x 4 of each; V: [layer] pieces of S x kv floats, the first n_pos x kv
    auto enqueue = [&]() -> int {
        HIP_OK(hipMemcpy2DAsync(b->k_of(dst_slot), S * 16, b->k_of(src_slot), S * 16, (size_t)n_pos * 16, (size_t)a.n_layers * kv / 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_OK(hipMemcpy2DAsync(b->v_of(dst_slot), S * kv * 4, b->v_of(src_slot), S * kv * 4, (size_t)n_pos * kv * 4, a.n_layers, hipMemcpyDeviceToDevice, c->stream));
        return history_fork(b, src_slot, dst_slot, n_pos);
    };
    if (enqueue()) return batch_failed(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

// The pinned long table (RunTable) of a pass over n_runs runs, the arguments checked by the caller: caller row j (run order, ascending position) behind table
// row r, deepest first; sel[o] = the table row of output o.  *rows / *outs: the table's rows and the outputs asked for.
// Where the rows of a ragged pass come from: kind[i] = 0, run i's rows are the next run_len[i] ids of `tokens`; 1, the next run_len[i] rows (dim floats each) of
// `embeddings`.  kind null: every run is a token run (the token entry points).  The table's `tok` column then carries a source word per row
// (source_rows_kernel below): the token id, or kRowFromStage | the row's place among the call's embedding rows.
struct RunRows { const uint32_t* kind; const uint32_t* tokens; const float* embeddings; };
static void runs_table(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len, const uint32_t* n_out,
                       RunRows src, size_t* rows_out, size_t* outs) {
    struct Row { uint32_t run, pos, word; };
    std::vector<Row> rows;
    uint32_t n_tok = 0, n_emb = 0;
    for (uint32_t i = 0; i < n_runs; ++i) for (uint32_t j = 0; j < (run_len ? run_len[i] : 1u); ++j)
        rows.push_back(Row{i, start_pos[i] + j, src.kind && src.kind[i] ? kRowFromStage | n_emb++ : src.tokens[n_tok++]});
    const size_t R = rows.size();
    std::vector<int> order(R), at(R);
    for (size_t j = 0; j < R; ++j) order[j] = (int)j;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return rows[x].pos > rows[y].pos; });
    RunTable* h = b->h_runs;
    for (size_t r = 0; r < R; ++r) {
        const int j = order[r];
        h->off[r] = b->off_of(slot[rows[j].run]); h->pos[r] = (int)rows[j].pos; h->tok[r] = rows[j].word;
        if (b->hist) b->h_hist_slot[r] = (int)slot[rows[j].run];
        at[j] = (int)r;
    }
    size_t o = 0;
    for (size_t i = 0, j = 0; i < n_runs; ++i) {
        const uint32_t len = run_len ? run_len[i] : 1u, no = n_out ? n_out[i] : 1u;
        for (uint32_t u = len - no; u < len; ++u) {
            if (b->n_masked) b->h_mask_of[o] = b->mask_row_of(slot[i]);     // (the classifier sees the outputs in this order)
            if (b->n_aut) b->h_aut_rows[o] = b->auto_row_of(slot[i]);
            if (b->n_pen) b->h_pen_of[o] = b->penalty_row_of(slot[i], at[j + u]);
            if (b->n_flt) b->h_flt_of[o] = b->filter_row_of(slot[i]);
            h->sel[o++] = (uint32_t)at[j + u];
        }
        j += len;
    }
    b->mask_live = false; b->pen_live = false; b->aut_live = false; b->flt_live = false;
    *rows_out = R; *outs = o;
}
// One pass over the device's long table as it stands: R rows through the layers, then the O rows of sel through the final norm and the classifier to
// their sink.  step: how far the rows have moved since runs_table (sizes the attention's score vector).  Every GEMM in the weight-streaming forms up to
// kStreamPassMax rows - the skinny kernel up to 16, the stream kernel above - and launch_gemm_q8's dispatch beyond.
// The rows of a ragged pass that has an embedding run (lmrs_batch_forward_runs_embed): one workgroup per table row, where launch_dequant_rows stands in a
// token-only pass.  (In this file, not beside dequant_rows_kernel: the code object of lmrs_kernels.hip - every kernel of the decode step and of the passes -
// stays byte for byte what it was; dequant_elem is shared through lmrs_device_math.h.)  src[r] without kRowFromStage is a token id - dequant_rows_kernel's loop and arithmetic, Gemma's one f32 multiply included; with it, the
// low bits name a row of the staged block (the caller's embedding rows, f32), copied as it is, 16 bytes a lane: fill_kv_cache takes its rows as given.
__global__ __launch_bounds__(256) void source_rows_kernel(const void* q, const float* s, int q4, const uint32_t* src, const float* staged, int dim, float* out,
                                                          float scale, int do_scale) {
    const uint32_t w = src[blockIdx.x];
    if (w & kRowFromStage) {
        const float4* from = reinterpret_cast<const float4*>(staged) + (size_t)(w & ~kRowFromStage) * (dim / 4);
        float4* to = reinterpret_cast<float4*>(out) + (size_t)blockIdx.x * (dim / 4);
        for (int i = threadIdx.x; i < dim / 4; i += blockDim.x) to[i] = from[i];
        return;
    }
    for (int i = threadIdx.x; i < dim; i += blockDim.x) {
        float v = dequant_elem(q, s, q4, (size_t)w * dim + i);
        if (do_scale) v = v * scale;                                        // (embed_kernel's multiply)
        out[(size_t)blockIdx.x * dim + i] = v;
    }
}
static hipError_t launch_source_rows(const void* q, const float* s, int q4, const uint32_t* src, const float* staged, int n_rows, int dim, float* out, hipStream_t st,
                              float scale) {
    if (n_rows < 1 || n_rows > kRunRowsMax || dim < 4 || dim % 4 || !staged) return hipErrorInvalidValue;
    hipLaunchKernelGGL(source_rows_kernel, dim3(n_rows), dim3(256), 0, st, q, s, q4, src, staged, dim, out, scale, scale != 0.0f ? 1 : 0);
    return hipGetLastError();
}
// staged: the pass has embedding rows, uploaded to that block - the rows come from launch_source_rows instead of token_rows
static int source_rows(lmrs_ctx* c, const uint32_t* src, const float* staged, int m) {       // token_rows with a source word per row
    const float scale = c->args.model_type == LMRS_GEMMA ? sqrtf((float)c->args.dim) : 0.0f;
    HIP_OK(launch_source_rows(c->emb_q, c->emb_s, c->q4, src, staged, m, (int)c->args.dim, c->pf_x, c->stream, scale));
    return 0;
}
static int runs_pass(lmrs_batch* b, size_t R, size_t O, uint32_t step, RowSink to, const float* staged = nullptr) {
    lmrs_ctx* c = b->c;
    PassForm form; form.skinny = R <= kStreamPassMax; form.runs = b->runs_view(); form.max_T = b->h_runs->pos[0] + (int)step + 1; form.qkv = b->runs_qkv;
    form.k_cache = b->kv; form.v_cache = b->kv + (b->pool ? b->page_floats : b->slot_floats); form.pages = b->page_view();
    if (record_rows(b, form.runs.pos, form.runs.tok, R)) return -1;
    if ((staged ? source_rows(c, form.runs.tok, staged, (int)R) : token_rows(c, form.runs.tok, (int)R)) || prefill_pass(c, form, (int)R, 0)) return -1;
    if (!O) return 0;                                    // K/V rows only: neither the final norm nor the classifier runs
    HIP_OK(launch_select_rows(c->pf_x, b->runs->sel, b->runs_x, (int)c->args.dim, (int)O, c->stream));
    PassForm cls; cls.skinny = O <= kStreamPassMax; cls.masks = b->mask_view(); cls.autos = b->auto_view(); cls.penalties = b->penalty_view(form.runs.pos, form.max_T); cls.filters = b->filter_view();
    to.targets = false;
    return classify_rows(c, cls, to, b->runs_x, 0, (int)O);
}

// The arguments of a step, checked before any device work; then the pinned row table, sorted by descending position (the deepest attention workgroups
// dispatch first; the order is the same for every pass of a call, all positions moving together): order[r] = the caller's row behind table row r
// cap: the most rows the call takes (the batch's width; 16 for the sampled step).  Above kRowTableMax rows the pass is the ragged one with runs of one
// token (runs_table: outputs in the caller's row order, `order` is not written)
static int batch_rows(lmrs_batch* b, const char* what, uint32_t cap, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos, uint32_t span, int* order) {
    const lmrs_ctx* c = b->c;
    if (n < 1 || n > cap) return fail(std::string(what) + ": n = " + std::to_string(n) + " is outside 1 .. " + std::to_string(cap));
    uint64_t seen = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (slot[i] >= b->n_slots) return fail(std::string(what) + ": row " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " of " + std::to_string(b->n_slots));
        if (seen >> slot[i] & 1u) return fail(std::string(what) + ": slot " + std::to_string(slot[i]) + " appears twice");
        seen |= uint64_t(1) << slot[i];
        if (tokens[i] >= c->args.vocab_size) return fail(std::string(what) + ": token " + std::to_string(i) + " out of range");
        if ((size_t)pos[i] + span > c->args.seq_len) return fail(std::string(what) + ": row " + std::to_string(i) + ": pos + " + std::to_string(span) + " positions exceeds seq_len");
        if (b->auto_exhausted(slot[i]))
            return fail(std::string(what) + ": row " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " stands in final state " + std::to_string(b->aut_q[slot[i]]) + " of its automaton, which allows no token");
    }
    if (n > (uint32_t)kRowTableMax) { size_t R, O; runs_table(b, n, slot, pos, nullptr, nullptr, RunRows{nullptr, tokens, nullptr}, &R, &O); return 0; }
    for (uint32_t i = 0; i < n; ++i) order[i] = (int)i;
    std::stable_sort(order, order + n, [&](int x, int y) { return pos[x] > pos[y]; });
    for (uint32_t r = 0; r < n; ++r) {
        const int i = order[r];
        b->h_tab->off[r] = b->off_of(slot[i]); b->h_tab->pos[r] = (int)pos[i]; b->h_tab->tok[r] = tokens[i];
        if (b->n_masked) b->h_mask_of[r] = b->mask_row_of(slot[i]);
        if (b->n_aut) b->h_aut_rows[r] = b->auto_row_of(slot[i]);
        if (b->hist) b->h_hist_slot[r] = (int)slot[i];
        if (b->n_pen) b->h_pen_of[r] = b->penalty_row_of(slot[i], (int)r);
        if (b->n_flt) b->h_flt_of[r] = b->filter_row_of(slot[i]);
    }
    b->mask_live = false; b->pen_live = false; b->aut_live = false; b->flt_live = false;
    return 0;
}
// The record's columns of a call beside its table (a batch without the record enqueues nothing here): the slot of every one of the table's R rows, and - only
// when one of the O output rows is penalised - the penalty column, which the pass's forms then carry (lmrs_batch::penalty_view)
static int record_enqueue(lmrs_batch* b, size_t R, size_t O) {
    if (!b->hist) return 0;
    HIP_OK(hipMemcpyAsync(b->hist_slot, b->h_hist_slot, R * sizeof(int), hipMemcpyHostToDevice, b->c->stream));
    if (!b->n_pen || !std::any_of(b->h_pen_of.get(), b->h_pen_of + O, [](const PenaltyRow& r) { return r.slot >= 0; })) return 0;
    HIP_OK(hipMemcpyAsync(b->pen_of, b->h_pen_of, O * sizeof(PenaltyRow), hipMemcpyHostToDevice, b->c->stream));
    b->pen_live = true;
    return 0;
}
// The mask column of a call with n output rows, beside its table: uploaded - and the pass's forms carry it (lmrs_batch::mask_view) - only when one of the
// rows is masked; a batch without masks enqueues nothing here
// filters: the filters' column too, in the same way (lmrs_batch_generate_greedy passes false: no filter moves an argmax, so its passes skip the launch)
static int masks_enqueue(lmrs_batch* b, size_t n, bool filters = true) {
    if (filters && b->n_flt && std::any_of(b->h_flt_of.get(), b->h_flt_of + n, [](const FilterRow& r) { return r.slot >= 0; })) {
        HIP_OK(hipMemcpyAsync(b->flt_of, b->h_flt_of, n * sizeof(FilterRow), hipMemcpyHostToDevice, b->c->stream));
        b->flt_live = true;
    }
    // the automata's column in the same way, and in front of it the state words where the host has moved one since they last went up
    if (b->n_aut && std::any_of(b->h_aut_rows.get(), b->h_aut_rows + n, [](const AutoRow& r) { return r.slot >= 0; })) {
        if (b->aut_dirty) {
            memcpy(b->h_aut_state, b->aut_q, b->n_slots * 4);
            HIP_OK(hipMemcpyAsync(b->aut_state, b->h_aut_state, b->n_slots * 4, hipMemcpyHostToDevice, b->c->stream));
            b->aut_dirty = false;
        }
        HIP_OK(hipMemcpyAsync(b->aut_rows, b->h_aut_rows, n * sizeof(AutoRow), hipMemcpyHostToDevice, b->c->stream));
        b->aut_live = true;
    }
    if (!b->n_masked || !std::any_of(b->h_mask_of.get(), b->h_mask_of + n, [](int m) { return m >= 0; })) return 0;
    HIP_OK(hipMemcpyAsync(b->mask_of, b->h_mask_of, n * sizeof(int), hipMemcpyHostToDevice, b->c->stream));
    b->mask_live = true;
    return 0;
}
// one pass over the device table's rows as they stand; step: how far the rows have moved since batch_rows (sizes the attention's score vector)
static int batch_pass(lmrs_batch* b, uint32_t n, uint32_t step, float* out_logits) {
    lmrs_ctx* c = b->c;
    PassForm form; form.skinny = true; form.rows = b->tab; form.max_T = b->h_tab->pos[0] + (int)step + 1; form.k_cache = b->kv; form.v_cache = b->kv + b->slot_floats;
    if (b->pool) { form.v_cache = b->kv + b->page_floats; form.pages = b->page_view(); }
    form.masks = b->mask_view(); form.autos = b->auto_view(); form.penalties = b->penalty_view(b->tab->pos, form.max_T); form.filters = b->filter_view();
    if (record_rows(b, b->tab->pos, b->tab->tok, n)) return -1;
    RowSink to{0, n, out_logits, 0}; to.targets = false;
    return run_tokens(c, to, form, /*batched=*/true);
}

extern "C" int lmrs_batch_forward(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos, uint32_t* argmax, float* logits) {
    if (!b || !slot || !tokens || !pos || !argmax) return fail("NULL argument");
    lmrs_ctx* c = b->c;
    int order[kRowTableMax];
    if (batch_rows(b, "lmrs_batch_forward", b->width, n, slot, tokens, pos, 1, order)) return -1;
    if (pages_claim_rows(b, "lmrs_batch_forward: ", n, slot, pos, nullptr, 1)) return -1;
    HIP_OK(hipSetDevice(c->device));
    const size_t V = c->args.vocab_size;
    if (n > (uint32_t)kRowTableMax) {                    // a wide step: the long table, outputs in the caller's order straight to their places
        const HostScores hs = host_scores(c);
        auto enqueue = [&]() -> int {
            HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
            if (masks_enqueue(b, n) || record_enqueue(b, n, n) || batch_state(c)) return -1;
            RowSink to{0, n, logits, 0}; to.reduce_too = true;
            if (runs_pass(b, n, n, 0, to)) return -1;
            HIP_OK(hipMemcpyAsync(hs.idx, c->sc_idx, n * 4, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        if (batch_call(c, enqueue)) return -1;
        memcpy(argmax, hs.idx, n * 4);
        return 0;
    }
    std::vector<float> rows(logits ? n * V : 0);         // the pass's rows in table order
    auto enqueue = [&]() -> int {
        HIP_OK(hipMemcpyAsync(b->tab, b->h_tab, sizeof(RowTable), hipMemcpyHostToDevice, c->stream));
        if (masks_enqueue(b, n) || record_enqueue(b, n, n) || batch_state(c)) return -1;
        if (batch_pass(b, n, 0, nullptr)) return -1;     // the reduction: sample_argmax of every row -> sc_idx
        if (logits && copy_out_rows(c, RowSink{0, n, rows.data(), 0}, c->sc_logits, cls_rows(c), (int)n, 0)) return -1;
        HIP_OK(hipMemcpyAsync(b->h_out, c->sc_idx, n * 4, hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    if (batch_call(c, enqueue)) return -1;
    for (uint32_t r = 0; r < n; ++r) {
        argmax[order[r]] = b->h_out[r];
        if (logits) memcpy(logits + (size_t)order[r] * V, rows.data() + (size_t)r * V, V * 4);
    }
    return 0;
}

extern "C" int lmrs_batch_generate_greedy(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos, uint32_t n_new,
                                          uint32_t* out_tokens, double* seconds) {
    if (!b || !slot || !tokens || !pos || (!out_tokens && n_new)) return fail("NULL argument");
    lmrs_ctx* c = b->c;
    int order[kRowTableMax];
    if (batch_rows(b, "lmrs_batch_generate_greedy", b->width, n, slot, tokens, pos, n_new ? n_new : 1, order)) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (b->aut_of[slot[i]] >= 0) return fail("lmrs_batch_generate_greedy: row " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + " has an automaton: its state moves in lmrs_batch_generate's loop only");
    if (!n_new) return 0;
    if (pages_claim_rows(b, "lmrs_batch_generate_greedy: ", n, slot, pos, nullptr, n_new)) return -1;     // all n_new steps up front: the device loop crosses page edges alone
    HIP_OK(hipSetDevice(c->device));
    const bool wide = n > (uint32_t)kRowTableMax;        // the long table: results in the caller's row order
    auto enqueue = [&]() -> int {
        if (wide) HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
        else HIP_OK(hipMemcpyAsync(b->tab, b->h_tab, sizeof(RowTable), hipMemcpyHostToDevice, c->stream));
        if (masks_enqueue(b, n, /*filters=*/false) || record_enqueue(b, n, n) || batch_state(c)) return -1;       // (the column once: the rows keep their order over the n_new steps)
        HIP_OK(hipEventRecord(c->ev0, c->stream));
        for (uint32_t j = 0; j < n_new && wide; ++j) {
            if (runs_pass(b, n, n, j, RowSink{0, n, nullptr, 0})) return -1;
            HIP_OK(launch_runs_advance(b->runs->pos, b->runs->tok, b->runs->sel, c->sc_idx, b->out + (size_t)j * n, (int)n, c->stream));
        }
        for (uint32_t j = 0; j < n_new && !wide; ++j) {
            // the pass, then its results -> out[j][..], the rows' next tokens, their positions + 1: nothing of a step crosses to the host
            if (batch_pass(b, n, j, nullptr)) return -1;
            HIP_OK(launch_table_advance(b->tab, c->sc_idx, b->out + (size_t)j * n, (int)n, c->stream));
        }
        HIP_OK(hipEventRecord(c->ev1, c->stream));
        HIP_OK(hipMemcpyAsync(b->h_out, b->out, (size_t)n_new * n * 4, hipMemcpyDeviceToHost, c->stream));
        return 0;
    };
    if (batch_call(c, enqueue)) return -1;
    for (uint32_t j = 0; j < n_new; ++j) for (uint32_t r = 0; r < n; ++r) out_tokens[(size_t)(wide ? r : (uint32_t)order[r]) * n_new + j] = b->h_out[(size_t)j * n + r];
    if (seconds) { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, c->ev0, c->ev1)); *seconds = ms * 1e-3; }
    return 0;
}

// ------------------------------------------------------------------ the sampled step: lmrs_batch_forward's pass, then Sampler::sample per row
// (per row Transformer::forward + Sampler::sample, sampler.rs:109-129, with the row's own sampler: bit for bit lmrs_forward_sample on a context that holds
// only that sequence).  Temperature-0 rows take the pass's reduction; the others go through launch_sample_rows over the logits block, in place - the two
// sequential chains of every row side by side on the device.  One transfer brings back each row's {token, n0} and the head of its candidates; sample_topp's
// persistent vector lives in the host sampler, so top-p rows finish there (lmrs_sampler_topp_pairs), a flat row through the device sort first.
extern "C" int lmrs_sampler_topp_pairs(lmrs_sampler* s, const void* pairs, size_t n0, uint32_t* next);
extern "C" int lmrs_sampler_topp_sorted_pairs(lmrs_sampler* s, const void* sorted_pairs, size_t n0, uint32_t* next);
static size_t sample_scratch_floats(size_t rows) { return rows * (kSampleRowsGrid + 1) + rows + rows * kSampleRowsGrid; }
static SampleRowsArgs sample_rows_args(float* rows, int n_rows, int ld, int n, const SampleRow* tab, const uint32_t* argmax, float* scratch, unsigned long long* out) {
    float* sum = scratch + (size_t)n_rows * (kSampleRowsGrid + 1);
    return SampleRowsArgs{rows, n_rows, ld, n, tab, argmax, scratch, sum, reinterpret_cast<unsigned*>(sum + n_rows), out};
}
// A sampling set for R rows (alloc_all: whole or absent, one that grows is made anew); oom: the call's out-of-memory message, from the result blocks' bytes and R
static int sample_set_alloc(const lmrs_ctx* c, SampleSet& s, size_t R, std::string (*oom)(size_t bytes, size_t rows)) {
    const size_t V = c->args.vocab_size, head = 1 + std::min<size_t>(V, c->sw.topp_sort_min);
    s.rows = 0;
    if (!alloc_all({{s.tab, R}, {s.h_tab, R}, {s.scratch, sample_scratch_floats(R)}, {s.h_heads, R * head}, {s.out, R * (V + 1)}})) {
        (void)hipGetLastError();
        return fail(oom(R * (V + 1) * 8, R));
    }
    s.rows = R; s.head_words = head;
    return 0;
}
// The samplers of a sampled call, checked before any device work (`what` opens every message, noun: "row" / "run"): i's parameters to par[i], topp[i] by
// sampler.rs:117-126, *sampled: some row has a temperature.  A NULL sampler is refused (need_all) or skipped - that run has no output
static int samplers_check(const lmrs_ctx* c, const std::string& what, const char* noun, bool need_all, uint32_t n, lmrs_sampler* const* samplers,
                          SampleRow* par, bool* topp, bool* sampled) {
    const size_t V = c->args.vocab_size;
    *sampled = false;
    for (uint32_t i = 0; i < n; ++i) {
        topp[i] = false;
        const std::string at = what + noun + " " + std::to_string(i) + ": ";
        if (!samplers[i]) { if (need_all) return fail(at + "the sampler is NULL"); continue; }
        uint32_t vs = 0;
        if (lmrs_sampler_info(samplers[i], &vs, &par[i].temperature, &par[i].top_p, &par[i].rnd)) return -1;
        if (vs != V) return fail(at + "the sampler was made for another vocabulary size (" + std::to_string(vs) + ", the model has " + std::to_string(V) + ")");
        topp[i] = par[i].temperature != 0.0f && !(par[i].top_p <= 0.0f || par[i].top_p >= 1.0f);         // sampler.rs:117-126
        *sampled = *sampled || par[i].temperature != 0.0f;
        // (a top-p sampler carries its candidate vector from call to call: two rows of one call cannot both be "the next call")
        for (uint32_t j = 0; j < i && topp[i]; ++j)
            if (samplers[j] == samplers[i]) return fail(at + "the top-p sampler of " + noun + " " + std::to_string(j) + " appears twice (it carries state from call to call)");
    }
    if (*sampled && cls_rows(c) != (int)V) return fail(what + "the classifier leaves the last vocab_size % 4 logits unwritten: no sampled pass for this vocabulary");
    return 0;
}
// The sampled tail of a pass whose n output rows stand in sc_logits: the sampler table up, launch_sample_rows over the rows in place, and THE transfer -
// every row's {token, n0} and the first head_words - 1 of its candidates
static int sample_enqueue(lmrs_ctx* c, const SampleSet& s, size_t n, int max_rows = kSampleRowsMax) {
    const size_t V = c->args.vocab_size, head = s.head_words;
    HIP_OK(hipMemcpyAsync(s.tab, s.h_tab, n * sizeof(SampleRow), hipMemcpyHostToDevice, c->stream));
    HIP_OK(launch_sample_rows(sample_rows_args(c->sc_logits, (int)n, (int)V, (int)V, s.tab, c->sc_idx, s.scratch, s.out), c->stream, max_rows));
    HIP_OK(hipMemcpy2DAsync(s.h_heads, head * 8, s.out, (V + 1) * 8, head * 8, n, hipMemcpyDeviceToHost, c->stream));
    return 0;
}
// a row's head in the pinned copy: its first word is {token in the low half, n0 in the high half}, the candidates follow
struct SampleHead { const unsigned long long* cand; uint32_t tok, n0; };
static SampleHead sample_head(const SampleSet& s, size_t row) { const unsigned long long* w = s.h_heads + row * s.head_words; return {w + 1, (uint32_t)w[0], (uint32_t)(w[0] >> 32)}; }

extern "C" int lmrs_batch_forward_sample(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos,
                                         lmrs_sampler* const* samplers, uint32_t* next) {
    const std::string what = "lmrs_batch_forward_sample: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (!slot || !tokens || !pos || !samplers || !next) return fail(what + "NULL array");
    lmrs_ctx* c = b->c;
    int order[kRowTableMax], at[kRowTableMax];
    if (batch_rows(b, "lmrs_batch_forward_sample", kRowTableMax, n, slot, tokens, pos, 1, order)) return -1;
    const size_t V = c->args.vocab_size;
    SampleRow par[kRowTableMax]; bool topp[kRowTableMax]; bool sampled = false;
    if (samplers_check(c, what, "row", /*need_all=*/true, n, samplers, par, topp, &sampled)) return -1;
    HIP_OK(hipSetDevice(c->device));
    if (sampled && !b->samp.rows && sample_set_alloc(c, b->samp, kRowTableMax, [](size_t bytes, size_t) {
            return "lmrs_batch_forward_sample: " + std::to_string(bytes) + " bytes of candidate buffers: out of memory"; })) return -1;
    if (pages_claim_rows(b, what, n, slot, pos, nullptr, 1)) return -1;
    for (uint32_t r = 0; r < n; ++r) { at[order[r]] = (int)r; if (sampled) b->samp.h_tab[r] = par[order[r]]; }
    auto enqueue = [&]() -> int {
        HIP_OK(hipMemcpyAsync(b->tab, b->h_tab, sizeof(RowTable), hipMemcpyHostToDevice, c->stream));
        if (masks_enqueue(b, n) || record_enqueue(b, n, n) || batch_state(c)) return -1;
        if (batch_pass(b, n, 0, nullptr)) return -1;     // the reduction: sample_argmax of every row -> sc_idx; the rows stay in sc_logits
        if (!sampled) { HIP_OK(hipMemcpyAsync(b->h_out, c->sc_idx, n * 4, hipMemcpyDeviceToHost, c->stream)); return 0; }
        return sample_enqueue(c, b->samp, n);
    };
    if (batch_call(c, enqueue)) return -1;
    if (!sampled) { for (uint32_t r = 0; r < n; ++r) next[order[r]] = b->h_out[r]; return 0; }
    for (uint32_t i = 0; i < n; ++i) {                   // in row order: the host samplers move as n calls of lmrs_forward_sample would move them
        const int r = at[i];
        const SampleHead h = sample_head(b->samp, (size_t)r);
        const uint32_t n0 = h.n0;
        if (!topp[i]) { next[i] = h.tok; continue; }
        if (n0 > V) return fail(what + "row " + std::to_string(i) + ": the device reported " + std::to_string(n0) + " candidates");
        if (n0 < c->sw.topp_sort_min || n0 == 0) {
            if (lmrs_sampler_topp_pairs(samplers[i], h.cand, n0, &next[i])) return fail(what + "row " + std::to_string(i) + ": " + g_err);
            continue;
        }
        // a flat row: the candidates' sort (sampler.rs:81) on the device, over the row's probabilities as they stand in the logits block - p / 1.0f is p, so
        // the keys are those of the probabilities the filter saw and the sort must find the same n0
        int N = sample_sort_min_n();
        while ((size_t)N < n0) N <<= 1;
        if (samp_sort_alloc(c, N, V)) return -1;
        const float cutoff = (1.0f - par[i].top_p) / (float)(V - 1);
        unsigned* count = reinterpret_cast<unsigned*>(c->samp_keys + c->samp_cap);
        auto sort = [&]() -> int {
            HIP_OK(launch_sample_topp_sort(c->sc_logits + (size_t)r * V, (int)V, 1.0f, cutoff, N, c->samp_keys, count, c->samp_pairs, c->stream));
            HIP_OK(hipMemcpyAsync(c->h_pairs, c->samp_pairs, (size_t)n0 * 8, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipMemcpyAsync(c->h_pairs + (size_t)c->samp_cap * 8, count, 4, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        if (sort()) return batch_failed(c);
        HIP_OK(hipStreamSynchronize(c->stream));
        unsigned dev_n0 = 0; memcpy(&dev_n0, c->h_pairs + (size_t)c->samp_cap * 8, 4);
        if (dev_n0 != n0) return fail(what + "row " + std::to_string(i) + ": the sort found " + std::to_string(dev_n0) + " top-p candidates, the filter " + std::to_string(n0));
        if (lmrs_sampler_topp_sorted_pairs(samplers[i], c->h_pairs, n0, &next[i])) return fail(what + "row " + std::to_string(i) + ": " + g_err);
    }
    return 0;
}

// ------------------------------------------------------------------ the ragged batch pass: runs of consecutive tokens, one run per slot, one weight pass
// (no reference counterpart: per row Transformer::forward on a cache that holds only the row's sequence, in position order).  run_tokens' batched arm with the
// long table: rows sorted by descending position, the GEMMs skinny up to 16 rows and launch_gemm_q8's dispatch above, the qkv block in a buffer of the
// batch's own; behind the layers the rows whose outputs were asked for are made consecutive and only they go through the final norm and the classifier.
static_assert(kRunRowsMax == kPrefillTokens, "a ragged pass is one chunk of the batched pass");
// The runs of a ragged pass, checked before any device work (`what` opens every message): *rows / *outs = the rows they hold and the outputs asked for
// src.kind != null (the calls that take embedding runs): *embeds = the rows of the embedding runs; a kind other than 0 / 1, and a NULL array whose kind is present, are refused
static int runs_check(const lmrs_batch* b, const std::string& what, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                      const uint32_t* n_out, RunRows src, size_t* rows, size_t* outs, size_t* embeds = nullptr) {
    const lmrs_args& a = b->c->args;
    if (n_runs < 1 || n_runs > b->width) return fail(what + "n_runs = " + std::to_string(n_runs) + " is outside 1 .. " + std::to_string(b->width));
    size_t R = 0, O = 0, E = 0;
    for (uint32_t i = 0; i < n_runs; ++i) {
        if (run_len[i] < 1) return fail(what + "run " + std::to_string(i) + ": run_len is 0");
        if ((R += run_len[i]) > (size_t)kRunRowsMax) return fail(what + "the runs hold more than " + std::to_string(kRunRowsMax) + " rows");
        if (src.kind && src.kind[i] > 1) return fail(what + "run " + std::to_string(i) + ": run_kind = " + std::to_string(src.kind[i]) + " is neither 0 (tokens) nor 1 (embeddings)");
        if (src.kind && src.kind[i]) E += run_len[i];
    }
    uint64_t seen = 0;
    for (uint32_t i = 0; i < n_runs; ++i) {
        const std::string run = what + "run " + std::to_string(i) + ": ";
        if (slot[i] >= b->n_slots) return fail(run + "slot " + std::to_string(slot[i]) + " of " + std::to_string(b->n_slots));
        if (seen >> slot[i] & 1u) return fail(what + "slot " + std::to_string(slot[i]) + " appears in more than one run");
        seen |= uint64_t(1) << slot[i];
        if (n_out[i] > run_len[i]) return fail(run + "n_out = " + std::to_string(n_out[i]) + " exceeds run_len = " + std::to_string(run_len[i]));
        if ((size_t)start_pos[i] + run_len[i] > a.seq_len) return fail(run + "start_pos + run_len exceeds seq_len");
        if (n_out[i] && b->auto_exhausted(slot[i]))
            return fail(run + "slot " + std::to_string(slot[i]) + " stands in final state " + std::to_string(b->aut_q[slot[i]]) + " of its automaton, which allows no token");
        O += n_out[i];
    }
    if (R > E && !src.tokens) return fail(what + "tokens is NULL with a token run present");
    if (E && !src.embeddings) return fail(what + "embeddings is NULL with an embedding run present");
    for (size_t j = 0; j < R - E; ++j) if (src.tokens[j] >= a.vocab_size) return fail(what + "token " + std::to_string(j) + " out of range");
    *rows = R; *outs = O;
    if (embeds) *embeds = E;
    return 0;
}
// the staged block of a pass with embedding rows, at the first call that has one
static int embed_stage_alloc(lmrs_batch* b, const std::string& what) {
    if (b->embed_stage) return 0;
    const size_t bytes = (size_t)kRunRowsMax * b->c->args.dim * 4;
    if (!b->embed_stage.alloc(bytes / 4)) {
        (void)hipGetLastError();
        return fail(what + std::to_string(bytes) + " bytes of staging for " + std::to_string(kRunRowsMax) + " embedding rows: out of memory");
    }
    return 0;
}
// lmrs_batch_forward_runs and lmrs_batch_forward_runs_embed: the arguments' NULL checks are the caller's, `what` opens every message
static int forward_runs_from(const std::string& what, lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                             const uint32_t* n_out, RunRows src, uint32_t* argmax, float* logits, uint32_t k, uint32_t* topk_idx, float* topk_logprob) {
    lmrs_ctx* c = b->c;
    const lmrs_args& a = c->args;
    size_t R = 0, O = 0, E = 0;
    if (runs_check(b, what, n_runs, slot, start_pos, run_len, n_out, src, &R, &O, &E)) return -1;
    if (k && topk_check_k(k, a.vocab_size)) return -1;
    if (k && (!topk_idx || !topk_logprob)) return fail(what + "k > 0 needs topk_idx and topk_logprob");
    if (O && !argmax) return fail(what + "argmax is NULL with " + std::to_string(O) + " output rows asked for");
    for (uint32_t i = 0; i < n_runs && k; ++i)            // a masked row has n_allowed candidates that are numbers
        if (n_out[i] && b->allowed_now(slot[i]) && k > b->allowed_now(slot[i]))
            return fail(what + "run " + std::to_string(i) + ": slot " + std::to_string(slot[i]) + ": k = " + std::to_string(k) + " exceeds the " + std::to_string(b->allowed_now(slot[i])) +
                        (b->automaton_of(slot[i]) ? " tokens its automaton's state allows (n_allowed)" : " tokens its mask allows (n_allowed)"));
    runs_table(b, n_runs, slot, start_pos, run_len, n_out, src, &R, &O);
    HIP_OK(hipSetDevice(c->device));
    if (k && O && topk_alloc(c, c->sc_rows, (int)k)) return -1;
    if (E && embed_stage_alloc(b, what)) return -1;
    if (pages_claim_rows(b, what, n_runs, slot, start_pos, run_len, 0)) return -1;
    const HostScores hs = host_scores(c);
    const size_t nk = O * k;
    auto enqueue = [&]() -> int {
        if (E) HIP_OK(hipMemcpyAsync(b->embed_stage, src.embeddings, E * a.dim * 4, hipMemcpyHostToDevice, c->stream));     // the call's embedding rows, in caller order
        HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
        if (masks_enqueue(b, O) || record_enqueue(b, R, O) || batch_state(c)) return -1;
        RowSink to{0, O, logits, k}; to.reduce_too = true;
        if (runs_pass(b, R, O, 0, to, E ? b->embed_stage : nullptr)) return -1;
        if (!O) return 0;
        HIP_OK(hipMemcpyAsync(hs.idx, c->sc_idx, O * 4, hipMemcpyDeviceToHost, c->stream));
        if (k) {
            HIP_OK(hipMemcpyAsync(c->h_tk, c->tk_idx, nk * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipMemcpyAsync(c->h_tk + nk * 4, c->tk_val, nk * 4, hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    if (batch_call(c, enqueue)) return -1;
    if (O) memcpy(argmax, hs.idx, O * 4);
    if (O && k) { memcpy(topk_idx, c->h_tk, nk * 4); memcpy(topk_logprob, c->h_tk + nk * 4, nk * 4); }
    return 0;
}
// A prompt chunk of a paged batch - m rows of one slot from p0 on - takes block attention over the page table by prefill_attention's rule (and from
// kPagedBlockMin rows on); the table pass otherwise, or when lmrs_batch_debug_prefill_table forced it
static bool paged_block_route(const lmrs_batch* b, uint32_t m, uint32_t p0) {
    return !b->pf_table && m >= kPagedBlockMin && prefill_block_route(b->c, (int)m, (int)p0);
}
extern "C" int lmrs_batch_prefill_form(const lmrs_batch* b, size_t n, uint32_t start_pos, uint32_t* n_chunks, uint32_t* n_block) {
    const std::string what = "lmrs_batch_prefill_form: ";
    if (!b || !n_chunks || !n_block) return fail(what + "NULL argument");
    if ((size_t)start_pos + n > b->c->args.seq_len) return fail(what + "start_pos + n = " + std::to_string((size_t)start_pos + n) + " exceeds seq_len = " + std::to_string(b->c->args.seq_len));
    uint32_t chunks = 0, block = 0;
    for (size_t i0 = 0; i0 < n; i0 += kPrefillTokens, ++chunks) {
        const uint32_t m = (uint32_t)std::min<size_t>(kPrefillTokens, n - i0), p0 = start_pos + (uint32_t)i0;
        // (a contiguous batch sends a call of ONE row through the table pass; a longer call's last chunk of one row fails the rule by itself)
        if (b->pool ? paged_block_route(b, m, p0) : n > 1 && prefill_block_route(b->c, (int)m, (int)p0)) ++block;
    }
    *n_chunks = chunks; *n_block = block;
    return 0;
}
extern "C" int lmrs_batch_debug_prefill_table(lmrs_batch* b, int force) {
    if (!b) return fail("lmrs_batch_debug_prefill_table: NULL argument");
    if (!b->pool) return fail("lmrs_batch_debug_prefill_table: not a paged batch (lmrs_batch_create_paged)");
    b->pf_table = force != 0;
    return 0;
}
static int paged_prefill(const std::string& what, lmrs_batch* b, uint32_t slot, const uint32_t* tokens, const float* embeddings, size_t n, uint32_t start_pos, float* residual) {
    lmrs_ctx* c = b->c;
    const size_t dim = c->args.dim;
    HIP_OK(hipSetDevice(c->device));
    if (embeddings && embed_stage_alloc(b, what)) return -1;
    const PageRange all{slot, start_pos, start_pos + (uint32_t)n};
    if (pages_claim(b, what, &all, 1)) return -1;        // every chunk's pages up front: short of pages the call changes nothing
    // Gemma-2's window, as the contiguous calls set it: per row for tokens (batch_state), the call's first position for every row of embeddings
    const int win = embeddings ? pass_win_base(c, start_pos, false) : pass_win_base(c, 0, true);
    const uint32_t kind = embeddings ? 1u : 0u;
    for (size_t i0 = 0; i0 < n; i0 += kRunRowsMax) {
        const uint32_t m = (uint32_t)std::min<size_t>(kRunRowsMax, n - i0), p0 = start_pos + (uint32_t)i0, n_out = residual ? m : 0u;
        size_t R = 0, O = 0;
        const bool block = paged_block_route(b, m, p0);
        if (block) {                                     // block attention: the table's rows in POSITION order (row r = position p0 + r), no outputs
            RunTable* h = b->h_runs;
            for (uint32_t r = 0; r < m; ++r) { h->off[r] = b->off_of(slot); h->pos[r] = (int)(p0 + r); h->tok[r] = embeddings ? kRowFromStage | r : tokens[i0 + r]; if (b->hist) b->h_hist_slot[r] = (int)slot; }
            b->mask_live = false; b->pen_live = false; b->aut_live = false; b->flt_live = false;
        } else runs_table(b, 1, &slot, &p0, &m, &n_out, RunRows{&kind, tokens ? tokens + i0 : nullptr, embeddings}, &R, &O);
        auto enqueue = [&]() -> int {
            if (embeddings) HIP_OK(hipMemcpyAsync(b->embed_stage, embeddings + i0 * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
            if (record_enqueue(b, m, 0) || set_state(c, embeddings ? start_pos : 0, 0, win)) return -1;
            if (block) {
                if (record_rows(b, b->runs->pos, b->runs->tok, m)) return -1;                // (the table pass records in runs_pass)
                // the GEMM forms of a contiguous batch's chunk (m >= 16: never the skinny ones), the qkv block and the scatter of the table pass
                PassForm form; form.runs = b->runs_view(); form.qkv = b->runs_qkv; form.k_cache = b->kv; form.v_cache = b->kv + b->page_floats;
                form.pages = b->page_view(); form.block_pos0 = (int)p0; form.block_row = slot;
                if ((embeddings ? source_rows(c, form.runs.tok, b->embed_stage, (int)m) : token_rows(c, form.runs.tok, (int)m)) || prefill_pass(c, form, (int)m, (int)p0)) return -1;
                if (residual) HIP_OK(hipMemcpyAsync(residual + i0 * dim, c->pf_x, (size_t)m * dim * 4, hipMemcpyDeviceToHost, c->stream));     // (position order already)
                return 0;
            }
            if (runs_pass(b, m, 0, 0, RowSink{0, 0, nullptr, 0}, embeddings ? b->embed_stage : nullptr)) return -1;
            if (residual) {                              // the table's rows are deepest first: sel puts them back in position order
                HIP_OK(launch_select_rows(c->pf_x, b->runs->sel, b->runs_x, (int)dim, (int)m, c->stream));
                HIP_OK(hipMemcpyAsync(residual + i0 * dim, b->runs_x, (size_t)m * dim * 4, hipMemcpyDeviceToHost, c->stream));
            }
            return 0;
        };
        if (batch_call(c, enqueue)) return -1;                   // (the pinned table is rewritten for the next chunk)
    }
    return 0;
}
extern "C" int lmrs_batch_forward_runs(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                       const uint32_t* n_out, const uint32_t* tokens, uint32_t* argmax, float* logits,
                                       uint32_t k, uint32_t* topk_idx, float* topk_logprob) {
    const std::string what = "lmrs_batch_forward_runs: ";
    if (!b || !slot || !start_pos || !run_len || !n_out || !tokens) return fail(what + "NULL argument");
    return forward_runs_from(what, b, n_runs, slot, start_pos, run_len, n_out, RunRows{nullptr, tokens, nullptr}, argmax, logits, k, topk_idx, topk_logprob);
}
// Runs of embedding rows beside runs of tokens (Transformer::fill_kv_cache, transformer.rs:672-684, one row at a time - forward_layer, :388-657, with
// the row as given - where a token run is Transformer::forward): the same pass, the rows' source apart
extern "C" int lmrs_batch_forward_runs_embed(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                             const uint32_t* n_out, const uint32_t* run_kind, const uint32_t* tokens, const float* embeddings,
                                             uint32_t* argmax, float* logits, uint32_t k, uint32_t* topk_idx, float* topk_logprob) {
    const std::string what = "lmrs_batch_forward_runs_embed: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (!slot || !start_pos || !run_len || !n_out || !run_kind) return fail(what + "NULL array");
    return forward_runs_from(what, b, n_runs, slot, start_pos, run_len, n_out, RunRows{run_kind, tokens, embeddings}, argmax, logits, k, topk_idx, topk_logprob);
}

// ------------------------------------------------------------------ the sampled ragged pass: lmrs_batch_forward_runs' pass, then Sampler::sample on the last row of every run
// (per run Transformer::forward over its tokens + Sampler::sample, sampler.rs:109-129, with the run's own sampler: bit for bit lmrs_forward_sample after the
// run's tokens on a context that holds only that sequence).  The O sampled rows stand in the logits block in run order (runs_table's sel), so
// launch_sample_rows takes them as lmrs_batch_forward_sample's rows, up to the batch's width of them; the flat top-p rows of the call - n0 known after the
// first synchronise - are sorted together (launch_cand_sort) behind ONE second synchronise.  The buffers are this call's own: lmrs_batch_forward_sample's
// stay as that call documents them.
// room for `rows` sampled rows (whole sixteens, the batch's width at the most): made anew when a call needs more rows than the set holds
static int runs_sample_alloc(lmrs_batch* b, size_t rows) {
    if (b->rs.rows >= rows) return 0;
    return sample_set_alloc(b->c, b->rs, std::min<size_t>(b->width, (rows + 15) / 16 * 16), [](size_t bytes, size_t R) {
        return "lmrs_batch_forward_runs_sample: " + std::to_string(bytes) + " bytes of candidate buffers for " + std::to_string(R) + " rows: out of memory"; });
}
// F rows of N keys on the device and their pinned copy (alloc_all), made anew when a call sorts more
static int cand_sort_alloc(lmrs_batch* b, size_t F, size_t N) {
    if (b->cs_words >= F * N) return 0;
    b->cs_words = 0;
    if (!alloc_all({{b->cs_keys, F * N}, {b->h_cs_pairs, F * N}})) {
        (void)hipGetLastError();
        return fail("lmrs_batch_forward_runs_sample: " + std::to_string(F * N * 8) + " bytes of sort buffers for " + std::to_string(F) + " flat top-p rows: out of memory");
    }
    b->cs_words = F * N;
    return 0;
}

// lmrs_batch_forward_runs_sample and lmrs_batch_forward_runs_embed_sample: the arguments' NULL checks are the caller's, `what` opens every message
static int forward_runs_sample_from(const std::string& what, lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                    RunRows src, lmrs_sampler* const* samplers, uint32_t* next) {
    lmrs_ctx* c = b->c;
    if (n_runs < 1 || n_runs > b->width) return fail(what + "n_runs = " + std::to_string(n_runs) + " is outside 1 .. " + std::to_string(b->width));
    uint32_t n_out[kWideBatchMax]; int out_of[kWideBatchMax];                    // out_of[i]: run i's row among the outputs (-1: none)
    size_t R = 0, O = 0, E = 0;
    for (uint32_t i = 0; i < n_runs; ++i) { n_out[i] = samplers[i] ? 1u : 0u; out_of[i] = samplers[i] ? (int)O++ : -1; }
    if (runs_check(b, what, n_runs, slot, start_pos, run_len, n_out, src, &R, &O, &E)) return -1;
    const size_t V = c->args.vocab_size;
    SampleRow par[kWideBatchMax]; bool topp[kWideBatchMax]; bool sampled = false;
    if (samplers_check(c, what, "run", /*need_all=*/false, n_runs, samplers, par, topp, &sampled)) return -1;
    if (O > (size_t)c->sc_rows) return fail(what + "the logits block holds " + std::to_string(c->sc_rows) + " rows of this vocabulary, " + std::to_string(O) + " outputs were asked for");
    runs_table(b, n_runs, slot, start_pos, run_len, n_out, src, &R, &O);
    HIP_OK(hipSetDevice(c->device));
    if (sampled && runs_sample_alloc(b, O)) return -1;
    if (E && embed_stage_alloc(b, what)) return -1;
    if (pages_claim_rows(b, what, n_runs, slot, start_pos, run_len, 0)) return -1;
    for (uint32_t i = 0; i < n_runs; ++i) { next[i] = 0; if (sampled && out_of[i] >= 0) b->rs.h_tab[out_of[i]] = par[i]; }
    const HostScores hs = host_scores(c);
    auto enqueue = [&]() -> int {
        if (E) HIP_OK(hipMemcpyAsync(b->embed_stage, src.embeddings, E * c->args.dim * 4, hipMemcpyHostToDevice, c->stream));
        HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
        if (masks_enqueue(b, O) || record_enqueue(b, R, O) || batch_state(c)) return -1;
        if (runs_pass(b, R, O, 0, RowSink{0, O, nullptr, 0}, E ? b->embed_stage : nullptr)) return -1;          // the reduction: sample_argmax of every output row -> sc_idx; the rows stay in sc_logits
        if (!O) return 0;
        if (!sampled) { HIP_OK(hipMemcpyAsync(hs.idx, c->sc_idx, O * 4, hipMemcpyDeviceToHost, c->stream)); return 0; }
        return sample_enqueue(c, b->rs, O, (int)b->width);
    };
    if (batch_call(c, enqueue)) return -1;
    if (!O) return 0;
    if (!sampled) { for (uint32_t i = 0; i < n_runs; ++i) if (out_of[i] >= 0) next[i] = hs.idx[out_of[i]]; return 0; }
    // the flat rows of the call (a top-p row with LMRS_TOPP_DEVICE_SORT_MIN candidates or more): one table, one sequence of launches, one synchronise
    CandSortArgs cs{}; int flat_of[kWideBatchMax]; size_t n0_max = 0;
    for (uint32_t i = 0; i < n_runs; ++i) {
        flat_of[i] = -1;
        if (!topp[i]) continue;
        const uint32_t n0 = sample_head(b->rs, (size_t)out_of[i]).n0;
        if (n0 > V) return fail(what + "run " + std::to_string(i) + ": the device reported " + std::to_string(n0) + " candidates");
        if (n0 < c->sw.topp_sort_min || n0 == 0) continue;
        flat_of[i] = cs.n_rows; cs.t.row[cs.n_rows] = (unsigned)out_of[i]; cs.t.n0[cs.n_rows] = n0; ++cs.n_rows;
        n0_max = std::max<size_t>(n0_max, n0);
    }
    if (cs.n_rows) {
        cs.N = sample_sort_min_n();
        while ((size_t)cs.N < n0_max) cs.N <<= 1;
        if (cand_sort_alloc(b, (size_t)cs.n_rows, (size_t)cs.N)) return -1;
        cs.src = b->rs.out + 1; cs.ld = V + 1; cs.keys = b->cs_keys;
        auto sort = [&]() -> int {
            HIP_OK(launch_cand_sort(cs, c->stream));
            for (int f = 0; f < cs.n_rows; ++f)
                HIP_OK(hipMemcpyAsync(b->h_cs_pairs + (size_t)f * cs.N, b->cs_keys + (size_t)f * cs.N, (size_t)cs.t.n0[f] * 8, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        if (sort()) return batch_failed(c);
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    for (uint32_t i = 0; i < n_runs; ++i) {              // in run order: the host samplers move as n_runs calls of lmrs_forward_sample would move them
        if (out_of[i] < 0) continue;
        const SampleHead h = sample_head(b->rs, (size_t)out_of[i]);
        if (!topp[i]) { next[i] = h.tok; continue; }
        const int rc = flat_of[i] < 0 ? lmrs_sampler_topp_pairs(samplers[i], h.cand, h.n0, &next[i])
                                      : lmrs_sampler_topp_sorted_pairs(samplers[i], b->h_cs_pairs + (size_t)flat_of[i] * cs.N, h.n0, &next[i]);
        if (rc) return fail(what + "run " + std::to_string(i) + ": " + g_err);
    }
    return 0;
}
extern "C" int lmrs_batch_forward_runs_sample(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                              const uint32_t* tokens, lmrs_sampler* const* samplers, uint32_t* next) {
    const std::string what = "lmrs_batch_forward_runs_sample: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (!slot || !start_pos || !run_len || !tokens || !samplers || !next) return fail(what + "NULL array");
    return forward_runs_sample_from(what, b, n_runs, slot, start_pos, run_len, RunRows{nullptr, tokens, nullptr}, samplers, next);
}
extern "C" int lmrs_batch_forward_runs_embed_sample(lmrs_batch* b, uint32_t n_runs, const uint32_t* slot, const uint32_t* start_pos, const uint32_t* run_len,
                                                    const uint32_t* run_kind, const uint32_t* tokens, const float* embeddings,
                                                    lmrs_sampler* const* samplers, uint32_t* next) {
    const std::string what = "lmrs_batch_forward_runs_embed_sample: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    if (!slot || !start_pos || !run_len || !run_kind || !samplers || !next) return fail(what + "NULL array");
    return forward_runs_sample_from(what, b, n_runs, slot, start_pos, run_len, RunRows{run_kind, tokens, embeddings}, samplers, next);
}

// ------------------------------------------------------------------ the device loop whose rows end one by one: lmrs_batch_generate
// (per row the loop of chat.rs:188-222 over Transformer::forward + Sampler::sample with a stop set and a budget: bit for bit the per-sequence calls on a
// context that holds only that sequence).  The passes are lmrs_batch_generate_greedy's; behind each stands ONE launch (launch_gen_advance) where that loop
// has its advance: it records the chosen token, tests it against the row's stop set and budget, and either moves the table row on or leaves it where it is.
// A row that has ended but is still in the table computes the row it computed last - same token, same position, same earlier K/V - so it writes the same
// K/V bits, the same record entry and the same logits and chooses the same token again (sample_mult too: rnd is a constant of the sampler): harmless, and
// nothing at or beyond its end is touched.  Every check_every passes the host looks at the rows' states and, where a row has ended, builds the table anew from
// the live rows alone, through batch_rows (the mask, record and penalty columns with it): rows are independent of each other in every GEMM form, so compaction
// changes no bit.
static_assert(kGenRowsMax == (int)kWideBatchMax && kGenStopMax == LMRS_STOP_MAX, "a state block per row of a wide batch, the header's stop set");
static_assert(kGenFinishFinal == LMRS_FINISH_FINAL && kAutoDead == LMRS_STATE_DEAD && kAutoFinalBit == kStateFinalBit, "the boundary launch's codes are the header's");
static int gen_alloc(lmrs_batch* b, const std::string& what, size_t lp_words) {
    if (!b->gen_st && !alloc_all({{b->gen_st, kWideBatchMax}, {b->h_gen_st, kWideBatchMax}, {b->gen_live, 1}, {b->h_gen_live, 1}})) {
        (void)hipGetLastError();
        return fail(what + "row state blocks: out of memory");
    }
    // the log-probabilities' block by need (n * M of this call; one that grows is made anew)
    if (lp_words > b->gen_lp.count() && !alloc_all({{b->gen_lp, lp_words}, {b->h_gen_lp, lp_words}})) {
        (void)hipGetLastError();
        return fail(what + std::to_string(lp_words * 4) + " bytes of log-probabilities (and as many pinned): out of memory");
    }
    return 0;
}
extern "C" int lmrs_sampler_candidates(const lmrs_sampler* s, void* pairs, int* ordered);
extern "C" int lmrs_sampler_set_candidates(lmrs_sampler* s, const void* pairs);
// The vectors of a call's nt top-p rows on the device (alloc_all: whole or absent, a call with more rows makes the set anew)
static int topp_alloc(lmrs_batch* b, const std::string& what, size_t nt) {
    const size_t V = b->c->args.vocab_size, N = (size_t)topp_sort_n(V), bytes = nt * (2 * V + N) * 8;       // (and nt * V * 8 pinned)
    if (nt <= b->topp_vecs) return 0;
    b->topp_vecs = 0;
    if (!alloc_all({{b->topp_state, nt * 2 * V}, {b->topp_keys, nt * N}, {b->h_topp, nt * V}, {b->topp_which, kWideBatchMax}, {b->h_topp_which, kWideBatchMax},
                    {b->topp_ext, 2 * kWideBatchMax}, {b->h_topp_ext, 2 * kWideBatchMax}, {b->topp_of, kWideBatchMax}, {b->h_topp_of, kWideBatchMax}})) {
        (void)hipGetLastError();
        return fail(what + std::to_string(bytes) + " bytes of candidate vectors and sort keys (and " + std::to_string(nt * V * 8) + " pinned) for " + std::to_string(nt) + " top-p rows: out of memory");
    }
    b->topp_vecs = nt;
    return 0;
}
// lmrs_batch_generate and lmrs_batch_generate_topp: one loop.  allow_topp: a top-p row's candidate vector travels to the device at the start, launch_topp_rows
// follows launch_sample_rows in every pass, and the vector goes back into the host sampler at the end
static int batch_generate_run(const char* name, bool allow_topp, lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos,
                              const uint32_t* max_new, const uint32_t* n_stop, const uint32_t* stop_tokens, lmrs_sampler* const* samplers, uint32_t check_every,
                              uint32_t* out_tokens, float* out_logprobs, uint32_t* n_out, uint32_t* finish, uint64_t* stats2, double* seconds) {
    const std::string what = std::string(name) + ": ";
    const auto t0 = std::chrono::steady_clock::now();
    if (!b) return fail(what + "NULL argument (the batch)");
    if (!slot || !tokens || !pos || !max_new || !out_tokens || !n_out || !finish) return fail(what + "NULL array");
    lmrs_ctx* c = b->c;
    const size_t V = c->args.vocab_size, T = c->args.seq_len;
    if (check_every == 0) return fail(what + "check_every is 0");
    // the rows as every step checks them (batch_rows: n, slots, tokens, one position each; the table it leaves is built again below) and the samplers as the
    // sampled calls check them (samplers_check: the ONE copy of those rules), then what only this call asks
    int order0[kRowTableMax];
    if (batch_rows(b, name, b->width, n, slot, tokens, pos, 1, order0)) return -1;
    GenRow row[kWideBatchMax]; SampleRow par[kWideBatchMax]; bool topp[kWideBatchMax] = {};
    for (uint32_t i = 0; i < n; ++i) par[i] = SampleRow{0.0f, 0.0f, 0.0f};               // a NULL entry: sample_argmax
    uint32_t M = 0; size_t at_stop = 0; bool sampled = false;
    if (samplers && samplers_check(c, what, "row", /*need_all=*/false, n, samplers, par, topp, &sampled)) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        const std::string at = what + "row " + std::to_string(i) + ": ";
        if (max_new[i] == 0) return fail(at + "max_new is 0");
        if ((size_t)pos[i] + max_new[i] > T) return fail(at + "pos + max_new = " + std::to_string((size_t)pos[i] + max_new[i]) + " exceeds seq_len = " + std::to_string(T));
        GenRow& g = row[i];
        g = GenRow{};
        g.live = 1; g.budget = max_new[i]; g.last = tokens[i];
        if (n_stop) {
            if (n_stop[i] > (uint32_t)LMRS_STOP_MAX) return fail(at + "n_stop = " + std::to_string(n_stop[i]) + " exceeds LMRS_STOP_MAX = " + std::to_string(LMRS_STOP_MAX));
            if (n_stop[i] && !stop_tokens) return fail(what + "n_stop given without stop_tokens");
            for (uint32_t k = 0; k < n_stop[i]; ++k) {
                g.stop[k] = stop_tokens[at_stop + k];
                if (g.stop[k] >= V) return fail(at + "stop token " + std::to_string(k) + " = " + std::to_string(g.stop[k]) + " is not below vocab_size = " + std::to_string(V));
            }
            g.n_stop = n_stop[i]; at_stop += n_stop[i];
        }
        // (sample_topp's stale candidate vector lives in the host sampler, sampler.rs:81: a loop with a top-p row cannot run a step without a host round trip)
        if (topp[i] && !allow_topp) return fail(at + "a top-p sampler (top_p = " + std::to_string(par[i].top_p) + ") cannot run in the device loop: its candidate vector lives in the host sampler");
        g.from_samp = par[i].temperature != 0.0f ? 1u : 0u;
        M = std::max(M, max_new[i]);
    }
    for (uint32_t i = 0; i < n; ++i) row[i].out_at = i * M;
    // the top-p rows' vectors, numbered in row order (tv[i]; hvec: their host copies, the upload's source and the download's target); one that is not
    // ordered would break the merge's rank argument - no call of this library leaves one (a NaN never passes p >= cutoff), an import can
    uint32_t tv[kWideBatchMax], nt = 0;
    for (uint32_t i = 0; i < n; ++i) tv[i] = topp[i] ? nt++ : kToppNoVec;
    for (uint32_t i = 0; i < n; ++i) {
        if (!topp[i]) continue;
        int ordered = 0;
        if (lmrs_sampler_candidates(samplers[i], nullptr, &ordered)) return -1;
        if (!ordered) return fail(what + "row " + std::to_string(i) + ": the top-p sampler's candidate vector is not in descending order (an import through lmrs_sampler_set_candidates, or a NaN): the device merge needs an ordered vector");
    }
    if ((sampled || out_logprobs) && cls_rows(c) != (int)V)
        return fail(what + "the classifier leaves the last vocab_size % 4 logits unwritten: neither sampled rows nor log-probabilities for this vocabulary");
    if ((sampled || out_logprobs) && n > (uint32_t)c->sc_rows)
        return fail(what + "the logits block holds " + std::to_string(c->sc_rows) + " rows of this vocabulary, " + std::to_string(n) + " rows were given");
    HIP_OK(hipSetDevice(c->device));
    if (gen_alloc(b, what, out_logprobs ? (size_t)n * M : 0)) return -1;
    if (sampled && b->gen.rows < n && sample_set_alloc(c, b->gen, std::min<size_t>(b->width, ((size_t)n + 15) / 16 * 16), allow_topp ? +[](size_t bytes, size_t R) {
            return "lmrs_batch_generate_topp: " + std::to_string(bytes) + " bytes of candidate buffers for " + std::to_string(R) + " rows: out of memory"; } : +[](size_t bytes, size_t R) {
            return "lmrs_batch_generate: " + std::to_string(bytes) + " bytes of candidate buffers for " + std::to_string(R) + " rows: out of memory"; })) return -1;
    if (nt && topp_alloc(b, what, nt)) return -1;
    if (sampled && out_logprobs && b->gen_logits_rows < n) {
        b->gen_logits_rows = 0;
        if (!b->gen_logits.alloc((size_t)n * V)) { (void)hipGetLastError(); return fail(what + std::to_string((size_t)n * V * 4) + " bytes for the sampled rows' copy of the logits: out of memory"); }
        b->gen_logits_rows = n;
    }
    if (pages_claim_rows(b, what, n, slot, pos, max_new, 0)) return -1;     // every row's whole budget up front: the device loop crosses page edges alone
    // the vectors up: a vector that is all zero, as created, is cleared in place; every vector starts in its block 0
    // (both blocks of a vector hold it at the start: a step rewrites a prefix of the other block and relies on the rest)
    if (nt) { HIP_OK(hipMemsetAsync(b->topp_which, 0, kWideBatchMax * 4, c->stream)); HIP_OK(hipMemsetAsync(b->topp_ext, 0, 2 * kWideBatchMax * 4, c->stream)); }
    for (uint32_t i = 0; i < n; ++i) {
        if (!topp[i]) continue;
        unsigned long long* h = b->h_topp + (size_t)tv[i] * V;
        unsigned long long* d = b->topp_state + (size_t)tv[i] * 2 * V;
        if (lmrs_sampler_candidates(samplers[i], h, nullptr)) return batch_failed(c);
        if (std::all_of(h, h + V, [](unsigned long long w) { return w == 0; })) HIP_OK(hipMemsetAsync(d, 0, 2 * V * 8, c->stream));
        else {
            HIP_OK(hipMemcpyAsync(d, h, V * 8, hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipMemcpyAsync(d + V, d, V * 8, hipMemcpyDeviceToDevice, c->stream));
        }
    }
    std::vector<uint32_t> live(n);
    for (uint32_t i = 0; i < n; ++i) live[i] = i;
    // rows whose slots have automata: the boundary launch moves their state words on the device, so however the call ends the host's states go up again
    // before the next pass that needs them (the walk below makes them the reported tokens' states; a call that fails leaves the start states)
    struct StatesMoved { lmrs_batch* b; bool on; ~StatesMoved() { if (on) b->aut_dirty = true; } } states_moved{b, false};
    for (uint32_t i = 0; i < n; ++i) states_moved.on = states_moved.on || b->aut_of[slot[i]] >= 0;
    uint64_t passes = 0, row_passes = 0;
    // the table of the live rows alone, each where it stands now; output o of the pass is live row (wide ? o : order[o]).  It is built anew only behind a look
    // that found a row ended: while every row is live the device's table and state blocks ARE the rows' state, and the next chunk is enqueued as it stands
    uint32_t ls[kWideBatchMax], lt[kWideBatchMax], lp[kWideBatchMax]; int order[kRowTableMax];
    bool rebuild = true, wide = false, samp = false, tp = false; int top = 0;
    while (!live.empty()) {
        const uint32_t nl = (uint32_t)live.size();
        for (uint32_t j = 0; j < nl; ++j) { const uint32_t i = live[j]; ls[j] = slot[i]; lt[j] = row[i].last; lp[j] = pos[i] + row[i].done; }
        auto row_of = [&](uint32_t o) { return live[wide ? o : (uint32_t)order[o]]; };
        if (rebuild) {
            if (batch_rows(b, name, b->width, nl, ls, lt, lp, 1, order)) return -1;
            wide = nl > (uint32_t)kRowTableMax; samp = false; tp = false;
            for (uint32_t o = 0; o < nl; ++o) { b->h_gen_st[o] = row[row_of(o)]; samp = samp || row[row_of(o)].from_samp; tp = tp || topp[row_of(o)]; }
            for (uint32_t o = 0; o < nl && tp; ++o) b->h_topp_of[o] = tv[row_of(o)];
            for (uint32_t o = 0; o < nl && samp; ++o) b->gen.h_tab[o] = par[row_of(o)];
            top = wide ? b->h_runs->pos[0] : b->h_tab->pos[0];             // the deepest live row at the build (the tables are sorted by descending position)
        }
        auto enqueue = [&]() -> int {
            if (rebuild) {
                if (wide) HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
                else HIP_OK(hipMemcpyAsync(b->tab, b->h_tab, sizeof(RowTable), hipMemcpyHostToDevice, c->stream));
                if (masks_enqueue(b, nl) || record_enqueue(b, nl, nl) || (!passes && batch_state(c))) return -1;
                HIP_OK(hipMemcpyAsync(b->gen_st, b->h_gen_st, nl * sizeof(GenRow), hipMemcpyHostToDevice, c->stream));
                if (samp) HIP_OK(hipMemcpyAsync(b->gen.tab, b->gen.h_tab, nl * sizeof(SampleRow), hipMemcpyHostToDevice, c->stream));
                if (tp) HIP_OK(hipMemcpyAsync(b->topp_of, b->h_topp_of, nl * 4, hipMemcpyHostToDevice, c->stream));
            }
            const GenPick pick{c->sc_idx, samp ? b->gen.out.get() : nullptr, V + 1};
            for (uint32_t k = 0; k < check_every; ++k) {
                // max_T from the deepest position a live row can stand at in this pass: a row never moves beyond its budget's last position
                uint32_t deepest = 0;
                for (uint32_t j = 0; j < nl; ++j) deepest = std::max(deepest, std::min(lp[j] + k, pos[live[j]] + max_new[live[j]] - 1));
                const uint32_t step = deepest - (uint32_t)top;
                if (wide ? runs_pass(b, nl, nl, step, RowSink{0, nl, nullptr, 0}) : batch_pass(b, nl, step, nullptr)) return -1;
                if (samp) {
                    // the samplers overwrite their rows: with log-probabilities asked for they work on a copy and the block stays as the reduction saw it
                    float* rows = c->sc_logits;
                    if (out_logprobs) {
                        HIP_OK(hipMemcpyAsync(b->gen_logits, c->sc_logits, (size_t)nl * V * 4, hipMemcpyDeviceToDevice, c->stream));
                        rows = b->gen_logits;
                    }
                    HIP_OK(launch_sample_rows(sample_rows_args(rows, (int)nl, (int)V, (int)V, b->gen.tab, c->sc_idx, b->gen.scratch, b->gen.out), c->stream, (int)b->width));
                    // the top-p rows' sort, merge and draw behind it; a row that has ended reads its live word and stands still, one without a
                    // candidate is marked ended (finish 2) before the advance sees it
                    uint32_t* st_words = reinterpret_cast<uint32_t*>(b->gen_st.get());
                    if (tp) HIP_OK(launch_topp_rows(ToppRowsArgs{b->gen.out, V + 1, b->gen.tab, b->topp_of, (int)nl, (int)V, b->topp_state, b->topp_which, b->topp_ext, b->topp_keys,
                                                                 topp_sort_n(V), st_words + offsetof(GenRow, live) / 4, st_words + offsetof(GenRow, finish) / 4,
                                                                 sizeof(GenRow) / 4, nullptr}, c->stream));
                }
                if (out_logprobs) HIP_OK(launch_gen_logprobs(b->gen_st, pick, c->sc_logits, (int)V, (int)V, c->sc_part, b->gen_lp, (int)nl, c->stream));
                // (aut_live: the table's build found a row with an automaton - the launch then also moves the slots' state words)
                HIP_OK(launch_gen_advance(b->gen_st, wide ? b->runs->pos : b->tab->pos, wide ? b->runs->tok : b->tab->tok, wide ? b->runs->sel : nullptr, pick, b->out,
                                          b->gen_live, (int)nl, c->stream, b->aut_live ? b->aut_rows.get() : nullptr, b->aut_live ? b->aut_state.get() : nullptr));
            }
            HIP_OK(hipMemcpyAsync(b->h_gen_st, b->gen_st, nl * sizeof(GenRow), hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipMemcpyAsync(b->h_gen_live, b->gen_live, 4, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        if (batch_call(c, enqueue)) return -1;
        passes += check_every; row_passes += (uint64_t)check_every * nl;
        std::vector<uint32_t> next;
        for (uint32_t o = 0; o < nl; ++o) { row[row_of(o)] = b->h_gen_st[o]; if (b->h_gen_st[o].live) next.push_back(row_of(o)); }
        if (next.size() != *b->h_gen_live) return fail(what + "the device counted " + std::to_string(*b->h_gen_live) + " live rows, their states show " + std::to_string(next.size()));
        rebuild = next.size() != nl;
        if (rebuild) { std::sort(next.begin(), next.end()); live.swap(next); }
    }
    auto results = [&]() -> int {
        HIP_OK(hipMemcpyAsync(b->h_out, b->out, (size_t)n * M * 4, hipMemcpyDeviceToHost, c->stream));
        if (out_logprobs) HIP_OK(hipMemcpyAsync(b->h_gen_lp, b->gen_lp, (size_t)n * M * 4, hipMemcpyDeviceToHost, c->stream));
        if (nt) {
            HIP_OK(hipMemcpyAsync(b->h_topp_which, b->topp_which, nt * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_OK(hipMemcpyAsync(b->h_topp_ext, b->topp_ext, nt * 2 * 4, hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    if (batch_call(c, results)) return -1;
    // the vectors back into their samplers: the pinned copies still hold them as they came, and a vector has changed only below its extent - that prefix
    // comes down.  Whatever the caller does with a sampler next continues exactly
    auto vectors = [&]() -> int {
        for (uint32_t v = 0; v < nt; ++v) {
            const size_t changed = std::min<size_t>(b->h_topp_ext[2 * v + 1], V);
            if (changed) HIP_OK(hipMemcpyAsync(b->h_topp + (size_t)v * V, b->topp_state + ((size_t)v * 2 + (b->h_topp_which[v] & 1u)) * V, changed * 8, hipMemcpyDeviceToHost, c->stream));
        }
        return 0;
    };
    if (nt && batch_call(c, vectors)) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (topp[i] && lmrs_sampler_set_candidates(samplers[i], b->h_topp + (size_t)tv[i] * V)) return -1;
    for (uint32_t i = 0; i < n; ++i) {
        n_out[i] = row[i].done;
        finish[i] = row[i].finish == 2 ? (uint32_t)LMRS_FINISH_NO_CANDIDATE : row[i].finish == kGenFinishFinal ? (uint32_t)LMRS_FINISH_FINAL : row[i].finish ? LMRS_FINISH_STOP : LMRS_FINISH_BUDGET;
        for (uint32_t j = 0; j < M; ++j) {
            out_tokens[(size_t)i * M + j] = j < row[i].done ? b->h_out[(size_t)i * M + j] : 0u;
            if (out_logprobs) out_logprobs[(size_t)i * M + j] = j < row[i].done ? b->h_gen_lp[(size_t)i * M + j] : 0.0f;
        }
    }
    // the automata's states: the walk of every row's reported tokens from its start state (the device moved the words of the rows that stayed live only)
    for (uint32_t i = 0; i < n; ++i) {
        const lmrs_batch::Automaton* a = b->automaton_of(slot[i]);
        if (!a) continue;
        uint32_t q = b->aut_q[slot[i]]; size_t walked = 0;
        const int rc = automaton_walk(name, a->tables((uint32_t)V), q, out_tokens + (size_t)i * M, row[i].done, &q, &walked);
        b->aut_q[slot[i]] = q;
        if (rc) return fail(what + "row " + std::to_string(i) + ": " + g_err + " (a row without a number among its allowed logits)");
    }
    if (stats2) { stats2[0] = passes; stats2[1] = row_passes; }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}
extern "C" int lmrs_batch_generate(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos, const uint32_t* max_new,
                                   const uint32_t* n_stop, const uint32_t* stop_tokens, lmrs_sampler* const* samplers, uint32_t check_every,
                                   uint32_t* out_tokens, float* out_logprobs, uint32_t* n_out, uint32_t* finish, uint64_t* stats2, double* seconds) {
    return batch_generate_run("lmrs_batch_generate", false, b, n, slot, tokens, pos, max_new, n_stop, stop_tokens, samplers, check_every, out_tokens, out_logprobs,
                              n_out, finish, stats2, seconds);
}
// The same loop with top-p rows admitted: their candidate vectors resident on the device for the length of the call (launch_topp_rows)
extern "C" int lmrs_batch_generate_topp(lmrs_batch* b, uint32_t n, const uint32_t* slot, const uint32_t* tokens, const uint32_t* pos, const uint32_t* max_new,
                                        const uint32_t* n_stop, const uint32_t* stop_tokens, lmrs_sampler* const* samplers, uint32_t check_every,
                                        uint32_t* out_tokens, float* out_logprobs, uint32_t* n_out, uint32_t* finish, uint64_t* stats2, double* seconds) {
    return batch_generate_run("lmrs_batch_generate_topp", true, b, n, slot, tokens, pos, max_new, n_stop, stop_tokens, samplers, check_every, out_tokens, out_logprobs,
                              n_out, finish, stats2, seconds);
}

// ------------------------------------------------------------------ embedding rows into a slot: ONE fill_kv_cache call (transformer.rs:672-684) on the slot's cache
// (lmrs_fill_kv_cache's batched arm with the slot's caches in the pass's form: the rows as given, the window on start_pos for every row, 512 rows a chunk;
// the residual rows come back only when asked for).  One row goes through the long table with an embedding row in it, as lmrs_batch_prefill's one token
// goes through the table pass.
extern "C" int lmrs_batch_prefill_embeddings(lmrs_batch* b, uint32_t slot, const float* embeddings, uint32_t n, uint32_t start_pos, float* residual) {
    const std::string what = "lmrs_batch_prefill_embeddings: ";
    if (!b) return fail(what + "NULL argument (the batch)");
    lmrs_ctx* c = b->c;
    const lmrs_args& a = c->args;
    if (n == 0) return fail(what + "no rows given (n == 0)");
    if (!embeddings) return fail(what + "NULL argument (embeddings)");
    if (slot >= b->n_slots) return fail(what + "slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    if ((size_t)start_pos + n > a.seq_len) return fail(what + "start_pos + n = " + std::to_string((size_t)start_pos + n) + " exceeds seq_len = " + std::to_string(a.seq_len));
    if (b->pool) return paged_prefill(what, b, slot, nullptr, embeddings, n, start_pos, residual);
    HIP_OK(hipSetDevice(c->device));
    const size_t dim = a.dim;
    const int win = pass_win_base(c, start_pos, false);
    if (n == 1) {
        const uint32_t one = 1, none = 0;
        size_t R = 0, O = 0;
        if (embed_stage_alloc(b, what)) return -1;
        runs_table(b, 1, &slot, &start_pos, &one, &none, RunRows{&one, nullptr, embeddings}, &R, &O);
        auto enqueue = [&]() -> int {
            HIP_OK(hipMemcpyAsync(b->embed_stage, embeddings, dim * 4, hipMemcpyHostToDevice, c->stream));
            HIP_OK(hipMemcpyAsync(b->runs, b->h_runs, sizeof(RunTable), hipMemcpyHostToDevice, c->stream));
            if (record_enqueue(b, 1, 0) || set_state(c, start_pos, 0, win)) return -1;
            if (runs_pass(b, 1, 0, 0, RowSink{0, 0, nullptr, 0}, b->embed_stage)) return -1;
            if (residual) HIP_OK(hipMemcpyAsync(residual, c->pf_x, dim * 4, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        return batch_call(c, enqueue);
    }
    auto enqueue = [&]() -> int {
        if (set_state(c, start_pos, 0, win)) return -1;
        if (b->hist) HIP_OK(hipMemsetAsync(b->hist_of(slot) + start_pos, 0xFF, (size_t)n * 4, c->stream));       // the record: embedding rows have no token
        PassForm form; form.skinny = n < kShortPassMax; form.k_cache = b->k_of(slot); form.v_cache = b->v_of(slot);
        auto upload_rows = [&](size_t i0, int m) -> int {
            HIP_OK(hipMemcpyAsync(c->pf_x, embeddings + i0 * dim, (size_t)m * dim * 4, hipMemcpyHostToDevice, c->stream));
            return 0;
        };
        auto download_rows = [&](size_t i0, int m) -> int {
            if (residual) HIP_OK(hipMemcpyAsync(residual + i0 * dim, c->pf_x, (size_t)m * dim * 4, hipMemcpyDeviceToHost, c->stream));
            return 0;
        };
        return prefill_chunks(c, form, start_pos, n, upload_rows, download_rows);
    };
    return batch_call(c, enqueue);
}

extern "C" int lmrs_batch_debug_kv(lmrs_batch* b, uint32_t slot, int which, uint32_t layer, uint32_t pos, float* out) {
    if (!b || !out) return fail("NULL argument");
    if (slot >= b->n_slots) return fail("lmrs_batch_debug_kv: slot " + std::to_string(slot) + " of " + std::to_string(b->n_slots));
    if (b->pool) {                                       // the row's page (the zero page where nothing was claimed), at its in-page position
        if (pos >= b->c->args.seq_len) return fail("bad layer / position");
        const uint32_t page = b->pool->row(slot)[pos / b->page_len];
        return debug_kv_row(b->c, b->page_k(page), b->page_v(page), which, layer, pos % b->page_len, out, b->page_len);
    }
    return debug_kv_row(b->c, b->k_of(slot), b->v_of(slot), which, layer, pos, out);
}

// ------------------------------------------------------------------ measurement hooks
// The GEMV launches of one decode step, in step order (per layer qkv, wo, w1w3, w2; then the classifier),
// so that the weight stream is the real one (1.27 GB for Llama-3.2-1B: nothing is re-served by the 256 MiB
// Infinity Cache), each launch carrying its own start/stop HIP events (hipExtLaunchKernelGGL) on the context's stream.
extern "C" int lmrs_bench_gemv(lmrs_ctx* c, int iters, double* us5, double* bytes5, int* count5) {
    if (!c || iters <= 0 || !us5 || !bytes5 || !count5) return fail("bad argument");
    if (c->world > 1 || c->comm || c->f32) return fail("lmrs_bench_gemv: single-GPU contexts with quantised weights only");
    HIP_OK(hipSetDevice(c->device));
    const lmrs_args& a = c->args;
    const int nl = (int)a.n_layers, n_launch = 4 * nl + 1;
    std::vector<hipEvent_t> ev(2 * (size_t)n_launch);
    for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    const double bpe = c->q4 ? 0.5 : 1.0;
    for (int k = 0; k < 5; ++k) { us5[k] = 0; bytes5[k] = 0; count5[k] = 0; }
    auto mk = [&](int which, int layer, GemvArgs& g, int& pro, int& epi) {
        const DevLayer& L = c->layers[layer];
        g = GemvArgs{}; pro = PRO_QUANT; epi = EPI_STORE;
        g.q4 = c->q4; g.eps = a.rms_norm_eps; g.add_unit = a.model_type == LMRS_GEMMA; g.st = c->st;
        g.att_dim = c->att_dim; g.kv_dim = c->kv_dim; g.seq_len = a.seq_len; g.layer = layer;
        const bool gemma = a.model_type == LMRS_GEMMA, fz = c->gemma_fused;     // same launches as enqueue_layer / enqueue_step
        switch (which) {
            case 0: g.wq = L.wqkv; g.ws = L.sqkv; g.n = a.dim; g.o = c->att_dim + 2 * c->kv_dim; g.xin = c->x; g.rms_w = L.rms_att;
                    g.out = c->q; g.k_raw = c->k_raw; g.v_cache = c->v_cache; pro = PRO_RMS_QUANT; epi = EPI_QKV;
                    if (fz && layer > 0) { g.xin = c->x2; g.delta = c->tmp; g.add_w = c->layers[layer - 1].rms_post_ffn; g.xout = c->x; pro = PRO_ADD_RMS_QUANT; }
                    break;
            case 1: g.wq = L.wo; g.ws = L.so; g.n = c->att_dim; g.o = a.dim; g.xin = c->att_out; g.out = gemma ? c->tmp : c->x; epi = gemma ? EPI_STORE : EPI_RESID; break;
            case 2: g.wq = L.w13; g.ws = L.s13; g.n = a.dim; g.o = 2 * a.hidden_dim; g.xin = c->x; g.rms_w = gemma ? L.rms_pre_ffn : L.rms_post_att; g.out = c->h;
                    pro = PRO_RMS_QUANT; epi = gemma ? EPI_GELU : EPI_SWIGLU;
                    if (fz) { g.delta = c->tmp; g.add_w = L.rms_post_att; g.xout = c->x2; pro = PRO_ADD_RMS_QUANT; }
                    break;
            case 3: g.wq = L.w2; g.ws = L.s2; g.n = a.hidden_dim; g.o = a.dim; g.xin = c->h; g.out = gemma ? c->tmp : c->x; epi = gemma ? EPI_STORE : EPI_RESID; break;
            default: g = cls_args(c); pro = fz ? PRO_ADD_RMS_QUANT : PRO_RMS_QUANT; epi = EPI_CLS; break;
        }
    };
    if (set_state(c, a.seq_len - 1, 0)) return -1;      // the V row the qkv epilogue scribbles on: the last one
    for (int it = -1; it < iters; ++it) {              // it == -1: untimed warm-up pass
        int i = 0;
        for (int l = 0; l <= nl; ++l)
            for (int which = (l < nl ? 0 : 4); which < (l < nl ? 4 : 5); ++which) {
                GemvArgs g; int pro, epi; mk(which, l < nl ? l : 0, g, pro, epi);
                set_gemv_launch_events(ev[2 * i], ev[2 * i + 1]);       // events ride on the dispatch itself
                const hipError_t le = launch_gemv(g, pro, epi, c->stream);
                set_gemv_launch_events(nullptr, nullptr);
                HIP_OK(le);
                ++i;
            }
        HIP_OK(hipStreamSynchronize(c->stream));
        if (it < 0) continue;
        i = 0;
        for (int l = 0; l <= nl; ++l)
            for (int which = (l < nl ? 0 : 4); which < (l < nl ? 4 : 5); ++which) {
                GemvArgs g; int pro, epi; mk(which, l < nl ? l : 0, g, pro, epi);
                float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
                us5[which] += (double)ms * 1e3; bytes5[which] += (double)g.o * g.n * (bpe + 4.0 / 128.0); count5[which] += 1;
                ++i;
            }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    return 0;
}

// The REAL decode step (the launches of the captured graph, in order, on the live state: real activations, real positions)
// replayed eagerly `iters` times with a (start, stop) event pair on every dispatch: the duration of each kernel of the step as it
// runs inside the step - after its real predecessor, on the real data.  Decoding continues from the context's current state:
// call it right after lmrs_generate_greedy; the tokens it produces are valid greedy tokens (and are discarded).
// kind: 0 qkv, 1 attention, 2 wo, 3 w1w3, 4 w2, 5 classifier, 6 argmax (+ next embedding row), 7 glue launches of the sharded /
// unfused forms (slice quantise, residual adds), 8 peer-to-peer exchanges (RCCL collectives cannot carry events: 0 there).
// Row-sharded contexts: every rank must call it (the exchanges wait for the peers).
extern "C" int lmrs_bench_step(lmrs_ctx* c, uint32_t pos, int iters, double* us9, double* bytes9, int* count9) {
    if (!c || iters <= 0 || !us9 || !bytes9 || !count9) return fail("bad argument");
    const bool sharded = c->comm || c->p2p;
    if (sharded ? !(c->comm || c->p2p_ready) : !primary_graph(c)) return fail("lmrs_bench_step: the context cannot run a step by itself");
    if ((size_t)pos + iters + 1 > c->args.seq_len) return fail("positions out of range");
    if (c->att_split_pos > 0 && (int)(pos + iters + 1) > c->att_split_pos) return fail("lmrs_bench_step: positions below the split-attention threshold only");
    HIP_OK(hipSetDevice(c->device));
    const lmrs_args& a = c->args;
    for (int k = 0; k < 9; ++k) { us9[k] = 0; bytes9[k] = 0; count9[k] = 0; }
    const double bpe = c->q4 ? 0.5 : 1.0, sc = bpe + 4.0 / 128.0, dim = a.dim, att = c->att_dim, kv = c->kv_dim, attf = c->att_full, hidf = a.hidden_dim;
    const double wbytes[9] = {dim * (att + 2 * kv) * sc, 0, attf * c->dim_l * sc, 2.0 * dim * c->hid_l * sc, hidf * c->dim_l * sc, (double)c->voc_l * dim * sc, 0, 0, 0};
    if (set_state(c, pos, 0)) return -1;
    const StepForm form = step_form_for(c, pos + iters);       // the launches of the graph the timed run replayed (the form of the last position)
    const bool merged = form.qa_mode != 0;
    auto one_step = [&]() -> int { return sharded ? enqueue_step_sharded(c, form) : enqueue_step(c, form); };
    // dry pass (also the untimed warm-up: the first eager launches pay one-off costs): how many launches does a step have?
    hipEvent_t dummy[2]; int dtag[1];
    HIP_OK(hipEventCreate(&dummy[0])); HIP_OK(hipEventCreate(&dummy[1]));
    set_launch_event_pool(dummy, 0, dtag);
    int rc = one_step();
    const int per_step = launch_event_pool_used();
    set_launch_event_pool(nullptr, 0);
    (void)hipEventDestroy(dummy[0]); (void)hipEventDestroy(dummy[1]);
    if (rc) return -1;
    HIP_OK(hipStreamSynchronize(c->stream));
    std::vector<hipEvent_t> ev(2 * (size_t)per_step); std::vector<int> tags(per_step, 0);
    for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    for (int it = 0; it < iters && !rc; ++it) {            // the dry pass was position `pos`; the timed ones follow it
        set_launch_event_pool(ev.data(), per_step, tags.data());
        rc = one_step();
        const int used = launch_event_pool_used();
        set_launch_event_pool(nullptr, 0);
        if (rc) break;
        HIP_OK(hipStreamSynchronize(c->stream));
        if (used != per_step) { rc = fail("lmrs_bench_step: the step did not have the expected number of launches"); break; }
        for (int i = 0; i < per_step; ++i) {
            float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]));
            const int kind = tags[i] >= 0 && tags[i] < 9 ? tags[i] : 7;
            us9[kind] += (double)ms * 1e3; count9[kind] += 1;
            const double att_bytes = 2.0 * kv * 4 * ((double)pos + it + 3);                       // attention: K and V rows up to this step's position (pos + 1 + it), read + the new row
            bytes9[kind] += kind == 1 ? att_bytes : wbytes[kind] + (kind == 0 && merged ? att_bytes : 0.0);   // merged launches: everything under the first kind
        }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (!rc && check_err(c)) rc = -1;
    return rc;
}

// Debug timeline (LMRS_DEBUG_TIMELINE=1 at lmrs_create): 8 stamps (100 MHz wall clock) per kernel node of the
// last replay of the step graph: [0..3] first workgroup, [4..7] last workgroup: start, prologue done, first pass, end.
extern "C" int lmrs_debug_timeline(lmrs_ctx* c, unsigned long long* out, int max_nodes, int* n_nodes) {
    if (!c || !c->dbg) return fail("debug timeline not enabled (set LMRS_DEBUG_TIMELINE=1 before lmrs_create)");
    HIP_OK(hipSetDevice(c->device));
    const int n = 5 * (int)c->args.n_layers + (c->cls_tail ? 1 : 2);
    const int m = n < max_nodes ? n : max_nodes;
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipMemcpy(out, c->dbg, (size_t)m * 8 * 8, hipMemcpyDeviceToHost));
    if (n_nodes) *n_nodes = m;
    return 0;
}

// Verification aid (no reference counterpart): one row of the KV cache in the reference's layout (transformer.rs:302-303, 413:
// kv_dim floats of layer `layer`, position `pos`).  V is stored that way; K is stored blocked for the score lanes
// ([kv head][head/4][seq_len][4], see attention_body) and is gathered back here.
// (page_len > 0: the caches are ONE page of a paged batch - the same layout with page_len in the place of seq_len, pos the in-page position)
static int debug_kv_row(lmrs_ctx* c, const float* k_cache, const float* v_cache, int which, uint32_t layer, uint32_t pos, float* out, uint32_t page_len) {
    if (which < 0 || which > 1 || layer >= c->args.n_layers || pos >= (page_len ? page_len : c->args.seq_len)) return fail("bad layer / position");
    HIP_OK(hipSetDevice(c->device));
    HIP_OK(hipStreamSynchronize(c->stream));
    const size_t S = page_len ? page_len : c->args.seq_len, hs = c->args.head_size, kv = (size_t)c->kv_dim, nkv = kv / hs;
    if (which == 1) { HIP_OK(hipMemcpy(out, v_cache + ((size_t)layer * S + pos) * kv, kv * 4, hipMemcpyDeviceToHost)); return 0; }
    const float* kl = k_cache + (size_t)layer * nkv * hs * S;
    for (size_t h = 0; h < nkv; ++h)
        HIP_OK(hipMemcpy2D(out + h * hs, 16, kl + h * hs * S + pos * 4, S * 16, 16, hs / 4, hipMemcpyDeviceToHost));   // hs/4 words of 4 dims, S*16 bytes apart
    return 0;
}
extern "C" int lmrs_debug_kv(lmrs_ctx* c, int which, uint32_t layer, uint32_t pos, float* out) {
    if (!c || !out) return fail("NULL argument");
    return debug_kv_row(c, c->k_cache, c->v_cache, which, layer, pos, out);
}

extern "C" int lmrs_last_fill_ms(const lmrs_ctx* c, double* ms) {
    if (!c || !ms) return fail("NULL argument");
    if (c->last_fill_ms < 0) return fail("no batched fill_kv_cache has run on this context");
    *ms = c->last_fill_ms;
    return 0;
}

extern "C" int lmrs_debug_inject(lmrs_ctx* c, int what, int a, int b) {
    if (!c) return fail("ctx is NULL");
    if (what == 0) { c->inj_fail_connect = 1; return 0; }
    if (what == 1) {
        if (!(c->comm || c->p2p)) return fail("not a row-sharded context");
        HIP_OK(hipSetDevice(c->device));
        HIP_OK(hipStreamSynchronize(c->stream));
        destroy_step_graphs(c);
        c->eager = true; c->inj_stall_seg = a; c->inj_stall_ticks = (long long)b * 100;          // 100 MHz wall clock
        return 0;
    }
    return fail("unknown injection");
}

extern "C" int lmrs_debug_gemm_tile(uint32_t n, uint32_t o, uint32_t n_tok, int q4, int* tile_rows, int* tile_tokens, int* waves) {
    if (!tile_rows || !tile_tokens || !waves) return fail("NULL argument");
    if (n == 0 || n % 256 || o == 0 || o % 16 || n_tok == 0) return fail("lmrs_debug_gemm_tile: n must be a positive multiple of 256, o of 16");
    *tile_rows = *tile_tokens = *waves = 0;                      // below 48 tokens: the direct kernels (a token tile would be mostly padding)
    if (n_tok >= 48) { const GemmTile t = gemm_q8_ring_tile((int)n, (int)o, (int)n_tok, q4 != 0); *tile_rows = t.tm; *tile_tokens = t.tn; *waves = t.waves; }
    return 0;
}

extern "C" int lmrs_step_info(const lmrs_ctx* c, uint32_t pos, int* n_launches, double* algo_bytes) {
    if (!c) return fail("ctx is NULL");
    const lmrs_args& a = c->args;
    const double bpe = c->f32 ? 4.0 - 4.0 / 128.0 : (c->q4 ? 0.5 : 1.0), dim = a.dim, att = c->att_dim, kv = c->kv_dim, hid = a.hidden_dim, V = a.vocab_size, L = a.n_layers;   // (f32: 4 bytes, no scales)
    const double n_norm = a.model_type == LMRS_GEMMA ? 4 : 2;
    // weights + scales once, norm weights, KV read/write at this position
    double b = L * ((dim * att + 2 * dim * kv + att * dim + 3 * dim * hid) * (bpe + 4.0 / 128.0) + n_norm * dim * 4) + V * dim * (bpe + 4.0 / 128.0) +
               dim * 4 + L * 2 * kv * 4 * ((double)pos + 2);
    if (algo_bytes) *algo_bytes = b;
    const StepForm f = step_form_for(c, pos);
    const int att_launches = f.split_chunks ? (f.split_merged ? 2 : 3) : (f.qa_mode ? 1 : 2);      // qkv + attention: merged | separate | the split form with / without its scores in the qkv launch
    if (n_launches) *n_launches = ((a.model_type == LMRS_GEMMA && !c->gemma_fused ? 5 : 3) + att_launches) * (int)a.n_layers + (c->cls_tail ? 1 : 2);
    return 0;
}

// ------------------------------------------------------------------ L2 free functions (unit parity)
namespace {
struct Scratch {          // RAII device buffers for the op entry points
    std::vector<DevBuf<char>> p;
    void* get(size_t bytes) { DevBuf<char> q; if (!q.alloc(bytes)) return nullptr; p.push_back(std::move(q)); return p.back().get(); }
};
int op_begin(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail("bad device index");
    HIP_OK(hipSetDevice(device));
    return 0;
}
}  // namespace

extern "C" int lmrs_op_matmul_q8(int device, float* xout, const int8_t* xq, const float* xs, const int8_t* wq, const float* ws,
                                 size_t n, size_t o, size_t gs, size_t sl) {
    if (op_begin(device)) return -1;
    if (gs != 128 || n % 128) return fail("group size must be 128 and n a multiple of it");
    Scratch S; const size_t G = n / 128;
    void *dx = S.get(sl * n), *dxs = S.get(sl * G * 4), *dw = S.get(o * n), *dws = S.get(o * G * 4), *dout = S.get(sl * o * 4);
    if (!dout) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, xq, sl * n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dxs, xs, sl * G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dw, wq, o * n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dws, ws, o * G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0, sl * o * 4));
    const size_t o4 = o / 4 * 4;                       // par_chunks_exact_mut(4): tail rows are never written
    if (sl > 1 && n % 256 == 0 && o % 16 == 0) {       // a token batch: the matrix-core kernel of the batched forward_layer
        GemmArgs g{}; g.wq = dw; g.ws = static_cast<float*>(dws); g.xq = static_cast<const int8_t*>(dx); g.xs = static_cast<const float*>(dxs);
        g.n = (int)n; g.o = (int)o; g.n_tok = (int)sl; g.out = static_cast<float*>(dout);
        HIP_OK(launch_gemm_q8(g, EPI_STORE, nullptr));
        HIP_OK(hipMemcpy(xout, dout, sl * o * 4, hipMemcpyDeviceToHost));
        return 0;
    }
    for (size_t t = 0; t < sl && o4; ++t) {
        GemvArgs g{}; g.wq = dw; g.ws = static_cast<float*>(dws); g.n = (int)n; g.o = (int)o4;
        g.xq_in = static_cast<char*>(dx) + t * n; g.xs_in = static_cast<float*>(dxs) + t * G; g.out = static_cast<float*>(dout) + t * o;
        HIP_OK(launch_gemv(g, PRO_PREQ, EPI_STORE, nullptr));
    }
    HIP_OK(hipMemcpy(xout, dout, sl * o * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lmrs_debug_w13_quant(int device, int8_t* hq, float* hs, const int8_t* xq, const float* xs, const int8_t* wq, const float* ws,
                                    size_t n, size_t o, size_t n_tok, int gemma) {
    if (op_begin(device)) return -1;
    if (!gemm_q8_hq_fused((int)n, (int)o, (int)n_tok, false)) return fail("this w1/w3 shape does not take the quantising epilogue");
    Scratch S; const size_t G = n / 128;
    void *dx = S.get(n_tok * n), *dxs = S.get(n_tok * G * 4), *dw = S.get(o * n), *dws = S.get(o * G * 4), *dq = S.get(n_tok * (o / 2)), *ds = S.get(n_tok * (o / 256) * 4);
    if (!ds) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, xq, n_tok * n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dxs, xs, n_tok * G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dw, wq, o * n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dws, ws, o * G * 4, hipMemcpyHostToDevice));
    GemmArgs g{}; g.wq = dw; g.ws = static_cast<float*>(dws); g.xq = static_cast<const int8_t*>(dx); g.xs = static_cast<const float*>(dxs);
    g.n = (int)n; g.o = (int)o; g.n_tok = (int)n_tok; g.hq = static_cast<int8_t*>(dq); g.hs = static_cast<float*>(ds);
    HIP_OK(launch_gemm_q8(g, gemma ? EPI_GELU_Q : EPI_SWIGLU_Q, nullptr));
    HIP_OK(hipMemcpy(hq, dq, n_tok * (o / 2), hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(hs, ds, n_tok * (o / 256) * 4, hipMemcpyDeviceToHost));
    return 0;
}

// lmrs_debug_gemm_skinny / lmrs_debug_gemm_wide behind their checks: the operands to the device, one launch (stream: gemm_stream_kernel at any n_tok it
// serves; else launch_gemm_q8's skinny dispatch), the rows back
static int debug_gemm_rows(int device, float* out, const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws, size_t n, size_t o, size_t n_tok, int q4, bool stream) {
    if (op_begin(device)) return -1;
    Scratch S; const size_t G = n / 128, wb = q4 ? n / 2 : n;
    // Q4_0: the activations arrive as the reference packs them (element 2b in the low nibble of byte b, biased by 8) and go to the device as the int8 (q - 8)
    // rows the batched pass keeps: de-interleaved within every 8 elements, evens then odds (rows_prologue_kernel)
    std::vector<int8_t> x8;
    if (q4) {
        x8.resize(n_tok * n);
        const uint8_t* xp = reinterpret_cast<const uint8_t*>(xq);
        for (size_t t = 0; t < n_tok; ++t)
            for (size_t e = 0; e < n; e += 8)
                for (size_t b = 0; b < 4; ++b) {
                    const uint8_t v = xp[t * (n / 2) + e / 2 + b];
                    x8[t * n + e + b] = (int8_t)((int)(v & 0x0F) - 8); x8[t * n + e + 4 + b] = (int8_t)((int)(v >> 4) - 8);
                }
    }
    void *dx = S.get(n_tok * n), *dxs = S.get(n_tok * G * 4), *dw = S.get(o * wb), *dws = S.get(o * G * 4), *dout = S.get(n_tok * o * 4);
    if (!dx || !dxs || !dw || !dws || !dout) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, q4 ? x8.data() : xq, n_tok * n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dxs, xs, n_tok * G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dw, wq, o * wb, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dws, ws, o * G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0, n_tok * o * 4));
    GemmArgs g{}; g.wq = dw; g.ws = static_cast<float*>(dws); g.xq = static_cast<const int8_t*>(dx); g.xs = static_cast<const float*>(dxs);
    g.n = (int)n; g.o = (int)o; g.n_tok = (int)n_tok; g.q4 = q4 ? 1 : 0; g.out = static_cast<float*>(dout); g.skinny = 1;
    HIP_OK(stream ? launch_gemm_stream_store(g, nullptr) : launch_gemm_q8(g, EPI_STORE, nullptr));
    HIP_OK(hipMemcpy(out, dout, n_tok * o * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int lmrs_debug_gemm_skinny(int device, float* out, const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                                      size_t n, size_t o, size_t n_tok, int q4) {
    if (!out || !xq || !xs || !wq || !ws) return fail("NULL argument");
    if (n == 0 || n % 256 || o == 0 || o % 16 || n_tok < 1 || n_tok > kShortPassMax) return fail("lmrs_debug_gemm_skinny: n must be a positive multiple of 256, o of 16, n_tok 1 .. 16");
    return debug_gemm_rows(device, out, xq, xs, wq, ws, n, o, n_tok, q4, false);
}
extern "C" int lmrs_debug_gemm_wide(int device, float* out, const int8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                                    size_t n, size_t o, size_t n_tok, int q4) {
    if (!out || !xq || !xs || !wq || !ws) return fail("lmrs_debug_gemm_wide: NULL argument");
    if (n == 0 || n % 256 || o == 0 || o % 16 || n_tok < 1 || n_tok > kWideBatchMax) return fail("lmrs_debug_gemm_wide: n must be a positive multiple of 256, o of 16, n_tok 1 .. 64");
    return debug_gemm_rows(device, out, xq, xs, wq, ws, n, o, n_tok, q4, true);
}

extern "C" int lmrs_op_matmul_q4(int device, float* xout, const uint8_t* xq, const float* xs, const uint8_t* wq, const float* ws,
                                 size_t n, size_t o, size_t gs) {
    if (op_begin(device)) return -1;
    if (gs != 128 || n % 128) return fail("group size must be 128 and n a multiple of it");
    Scratch S; const size_t G = n / 128;
    void *dx = S.get(n / 2), *dxs = S.get(G * 4), *dw = S.get(o * n / 2), *dws = S.get(o * G * 4), *dout = S.get(o * 4);
    if (!dout) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, xq, n / 2, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dxs, xs, G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dw, wq, o * n / 2, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dws, ws, o * G * 4, hipMemcpyHostToDevice));
    GemvArgs g{}; g.q4 = 1; g.wq = dw; g.ws = static_cast<float*>(dws); g.n = (int)n; g.o = (int)o;
    g.xq_in = dx; g.xs_in = static_cast<float*>(dxs); g.out = static_cast<float*>(dout);
    HIP_OK(launch_gemv(g, PRO_PREQ, EPI_STORE, nullptr));
    HIP_OK(hipMemcpy(xout, dout, o * 4, hipMemcpyDeviceToHost));
    return 0;
}

static int op_quant(int device, void* q, float* s, const float* x, size_t n, size_t gs, int q4) {
    if (op_begin(device)) return -1;
    if (gs != 128 || n % 128) return fail("group size must be 128 and n a multiple of it");
    Scratch S; const size_t qb = q4 ? n / 2 : n;
    const size_t chunk = 8192;                         // one workgroup quantises up to 10240 elements; groups are independent
    void *dx = S.get(n * 4), *dq = S.get(qb), *ds = S.get(n / 128 * 4);
    if (!ds) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
    for (size_t e0 = 0; e0 < n; e0 += chunk) {
        const size_t m = n - e0 < chunk ? n - e0 : chunk;
        HIP_OK(launch_quantize(static_cast<float*>(dx) + e0, static_cast<char*>(dq) + (q4 ? e0 / 2 : e0), static_cast<float*>(ds) + e0 / 128, (int)m, q4, nullptr));
    }
    HIP_OK(hipMemcpy(q, dq, qb, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(s, ds, n / 128 * 4, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int lmrs_op_quantize(int device, int8_t* q, float* s, const float* x, size_t n, size_t gs) { return op_quant(device, q, s, x, n, gs, 0); }
extern "C" int lmrs_op_quantize_q4(int device, uint8_t* q, float* s, const float* x, size_t n, size_t gs) { return op_quant(device, q, s, x, n, gs, 1); }

extern "C" int lmrs_op_rmsnorm(int device, float* o, const float* x, const float* weight, size_t size, float eps, int add_unit_offset) {
    if (op_begin(device)) return -1;
    Scratch S; void *dx = S.get(size * 4), *dw = S.get(size * 4), *dout = S.get(size * 4);
    if (!dout) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, x, size * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dw, weight, size * 4, hipMemcpyHostToDevice));
    HIP_OK(launch_rmsnorm(static_cast<float*>(dx), static_cast<float*>(dw), static_cast<float*>(dout), (int)size, eps, add_unit_offset, nullptr));
    HIP_OK(hipMemcpy(o, dout, size * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lmrs_op_softmax(int device, float* x, size_t n) {
    if (op_begin(device)) return -1;
    if (n == 0) return fail("empty input (the reference indexes x[0])");
    Scratch S; void* dx = S.get(n * 4);
    if (!dx) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
    HIP_OK(launch_softmax(static_cast<float*>(dx), (int)n, nullptr));
    HIP_OK(hipMemcpy(x, dx, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// The classifier launch of the decode step (final rmsnorm + quantise | Q8_0 rows | logits + per-workgroup argmax partials)
// followed by the final argmax kernel, on caller-supplied rows: transformer.rs:341-381 + Sampler::sample_argmax (sampler.rs:29-41).
// For the edge cases the whole-model tests cannot reach (ties, NaN at index 0, NaN elsewhere, nothing above -inf).
extern "C" int lmrs_op_classifier_argmax(int device, const float* x, const float* rms_w, const int8_t* wq, const float* ws, size_t n, size_t o,
                                         float eps, uint32_t* token, float* logits) {
    if (op_begin(device)) return -1;
    if (!x || !rms_w || !wq || !ws || !token) return fail("NULL argument");
    if (n % 256 || n == 0 || n > 10240 || o == 0 || o % 4) return fail("n must be a multiple of 256 (<= 10240) and o a multiple of 4");
    Scratch S; const size_t G = n / 128;
    void *dx = S.get(n * 4), *dw = S.get(n * 4), *dq = S.get(o * n), *ds = S.get(o * G * 4), *dl = S.get(o * 4), *pv = S.get(kMaxArgmaxParts * 4), *pi = S.get(kMaxArgmaxParts * 4);
    void *dtok = S.get(16), *dst = S.get(sizeof(DevState));
    if (!dst) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dw, rms_w, n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dq, wq, o * n, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(ds, ws, o * G * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dtok, 0, 16)); HIP_OK(hipMemset(dst, 0, sizeof(DevState)));
    GemvArgs g{};
    g.wq = dq; g.ws = static_cast<float*>(ds); g.n = (int)n; g.o = (int)o; g.xin = static_cast<float*>(dx); g.rms_w = static_cast<float*>(dw); g.eps = eps;
    g.out = static_cast<float*>(dl); g.part_val = static_cast<float*>(pv); g.part_idx = static_cast<int*>(pi); g.st = static_cast<DevState*>(dst);
    const int grid = gemv_grid(g, PRO_RMS_QUANT, EPI_CLS);
    ArgmaxArgs m{};
    m.part_val = g.part_val; m.part_idx = g.part_idx; m.n_part = grid; m.n_groups = 1; m.logits = g.out; m.tokens = static_cast<uint32_t*>(dtok); m.st = static_cast<DevState*>(dst);
    m.emb.dim = 0; m.tail_row = 0;                      // no embedding row to prepare; o % 4 == 0
    // both forms the decode step uses: two launches (row-sharded steps), and the argmax folded into the classifier launch (one GPU);
    // they must agree - the folded form's answer is returned
    HIP_OK(launch_gemv(g, PRO_RMS_QUANT, EPI_CLS, nullptr));
    HIP_OK(launch_argmax_final(m, nullptr));
    uint32_t tk[2], tk2[2];
    HIP_OK(hipMemcpy(tk2, dtok, 8, hipMemcpyDeviceToHost));
    void *ppk = S.get(kMaxArgmaxParts * 8), *ptk = S.get(16);
    if (!ptk) return fail("hipMalloc failed");
    HIP_OK(hipMemset(ppk, 0, kMaxArgmaxParts * 8)); HIP_OK(hipMemset(ptk, 0, 16)); HIP_OK(hipMemset(dtok, 0, 16)); HIP_OK(hipMemset(dst, 0, sizeof(DevState)));
    g.has_tail = 1; g.tail.part_pk = static_cast<unsigned long long*>(ppk); g.tail.err = static_cast<int*>(ptk) + 1; m.seq = static_cast<unsigned*>(ptk); g.tail.cls_seq = static_cast<unsigned*>(ptk) + 2; g.tail.m = m;
    HIP_OK(launch_gemv(g, PRO_RMS_QUANT, EPI_CLS, nullptr));
    HIP_OK(hipMemcpy(tk, dtok, 8, hipMemcpyDeviceToHost));
    { int e2[2]; HIP_OK(hipMemcpy(e2, ptk, 8, hipMemcpyDeviceToHost)); if (e2[1]) return fail("classifier argmax: the folded form's consumer timed out"); }
    if (tk[1] != tk2[1]) return fail("classifier argmax: the folded form answered " + std::to_string(tk[1]) + ", the two-launch form " + std::to_string(tk2[1]));
    *token = tk[1];                                     // tokens[pos + 1] with pos = 0, prompt_end = 0
    if (logits) HIP_OK(hipMemcpy(logits, dl, o * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lmrs_op_sample_mult(int device, float* logits, size_t n, float temperature, float rnd, uint32_t* token) {
    if (op_begin(device)) return -1;
    if (!logits || !token || n == 0 || temperature == 0.0f) return fail("bad argument (temperature 0 is sample_argmax: lmrs_op_classifier_argmax)");
    Scratch S; void *dl = S.get(n * 4), *dp = S.get((kSampleGrid + 8) * 4);
    if (!dp) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dl, logits, n * 4, hipMemcpyHostToDevice));
    SampleArgs sa{static_cast<float*>(dl), (int)n, temperature, static_cast<float*>(dp)};
    HIP_OK(launch_sample_exps(sa, nullptr));
    HIP_OK(hipMemcpy(logits, dl, n * 4, hipMemcpyDeviceToHost));
    // the chains, as lmrs_sampler_sample_exps runs them for a sample_mult sampler (functional.rs:134-139, sampler.rs:43-55), with the caller's random number
    float sum = 0.0f;
    for (size_t i = 0; i < n; ++i) sum = sum + logits[i];
    for (size_t i = 0; i < n; ++i) logits[i] = logits[i] / sum;
    float cdf = 0.0f; *token = (uint32_t)(n - 1);
    for (size_t i = 0; i < n; ++i) { cdf = cdf + logits[i]; if (rnd < cdf) { *token = (uint32_t)i; break; } }
    return 0;
}

// launch_sample_rows on caller-supplied rows (unit parity against Sampler::sample on the same logits): the rows become the probabilities of their softmax
// (temperature 0: untouched), token[r] for sample_mult rows, n0[r] and pairs[r * n ..] - {f32 prob, u32 index} in index order - for top-p rows
extern "C" int lmrs_op_sample_rows(int device, float* rows, size_t n_rows, size_t n, const float* temperature, const float* top_p, const float* rnd,
                                   uint32_t* token, uint32_t* n0, void* pairs) {
    if (!rows || !temperature || !top_p || !rnd || !token || !n0) return fail("lmrs_op_sample_rows: NULL argument");
    if (n_rows < 1 || n_rows > (size_t)kSampleRowsMax) return fail("lmrs_op_sample_rows: n_rows = " + std::to_string(n_rows) + " is outside 1 .. " + std::to_string(kSampleRowsMax));
    if (n < 1 || n > (size_t)0x7FFFFFFF / 2) return fail("lmrs_op_sample_rows: need 1 <= n < 2^30");
    if (op_begin(device)) return -1;
    Scratch S;
    void *dl = S.get(n_rows * n * 4), *dt = S.get(n_rows * sizeof(SampleRow)), *ds = S.get(sample_scratch_floats(n_rows) * 4), *dout = S.get(n_rows * (n + 1) * 8);
    if (!dl || !dt || !ds || !dout) return fail("hipMalloc failed");
    std::vector<SampleRow> tab(n_rows);
    for (size_t r = 0; r < n_rows; ++r) tab[r] = SampleRow{temperature[r], top_p[r], rnd[r]};
    HIP_OK(hipMemcpy(dl, rows, n_rows * n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dt, tab.data(), n_rows * sizeof(SampleRow), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dout, 0, n_rows * (n + 1) * 8));
    HIP_OK(launch_sample_rows(sample_rows_args(static_cast<float*>(dl), (int)n_rows, (int)n, (int)n, static_cast<const SampleRow*>(dt), nullptr,
                                               static_cast<float*>(ds), static_cast<unsigned long long*>(dout)), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rows, dl, n_rows * n * 4, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n_rows; ++r) {
        unsigned long long h = 0;
        const char* blk = static_cast<const char*>(dout) + r * (n + 1) * 8;
        HIP_OK(hipMemcpy(&h, blk, 8, hipMemcpyDeviceToHost));
        token[r] = (uint32_t)h; n0[r] = (uint32_t)(h >> 32);
        if (n0[r] > n) return fail("lmrs_op_sample_rows: row " + std::to_string(r) + ": the device reported " + std::to_string(n0[r]) + " candidates");
        if (pairs && n0[r]) HIP_OK(hipMemcpy(static_cast<char*>(pairs) + r * n * 8, blk + 8, (size_t)n0[r] * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

// launch_cand_sort on caller-supplied candidates (unit parity against a stable sort by descending probability): ONE call of the launcher over every
// row with candidates, the rows padded to the power of two that holds the longest
static_assert(kCandSortRowsMax == (int)kWideBatchMax, "the flat rows of a call are at most a wide batch's runs");
extern "C" int lmrs_op_sort_candidates(int device, const void* pairs, size_t n_rows, size_t ld, const uint32_t* n0, void* sorted) {
    const std::string what = "lmrs_op_sort_candidates: ";
    if (!pairs || !n0 || !sorted) return fail(what + "NULL argument");
    if (n_rows < 1 || n_rows > (size_t)kCandSortRowsMax) return fail(what + "n_rows = " + std::to_string(n_rows) + " is outside 1 .. " + std::to_string(kCandSortRowsMax));
    if (ld < 1 || ld > ((size_t)1 << 24)) return fail(what + "need 1 <= ld <= 2^24");
    CandSortArgs cs{}; size_t n0_max = 0;
    for (size_t r = 0; r < n_rows; ++r) {
        if (n0[r] > ld) return fail(what + "row " + std::to_string(r) + ": n0 = " + std::to_string(n0[r]) + " exceeds ld = " + std::to_string(ld));
        if (!n0[r]) continue;
        cs.t.row[cs.n_rows] = (unsigned)r; cs.t.n0[cs.n_rows] = n0[r]; ++cs.n_rows;
        n0_max = std::max<size_t>(n0_max, n0[r]);
    }
    if (!cs.n_rows) return 0;
    if (op_begin(device)) return -1;
    cs.N = sample_sort_min_n();
    while ((size_t)cs.N < n0_max) cs.N <<= 1;
    Scratch S;
    void *dp = S.get(n_rows * ld * 8), *dk = S.get((size_t)cs.n_rows * cs.N * 8);
    if (!dp || !dk) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dp, pairs, n_rows * ld * 8, hipMemcpyHostToDevice));
    cs.src = static_cast<const unsigned long long*>(dp); cs.ld = ld; cs.keys = static_cast<unsigned long long*>(dk);
    HIP_OK(launch_cand_sort(cs, nullptr));
    HIP_OK(hipDeviceSynchronize());
    for (int f = 0; f < cs.n_rows; ++f)
        HIP_OK(hipMemcpy(static_cast<char*>(sorted) + (size_t)cs.t.row[f] * ld * 8, cs.keys + (size_t)f * cs.N, (size_t)cs.t.n0[f] * 8, hipMemcpyDeviceToHost));
    return 0;
}

// launch_automaton_masks on caller-supplied tables (unit parity against a host count): the tables' ranges are checked - the kernel indexes by them - the
// rule about non-final states is not
extern "C" int lmrs_op_automaton_masks(int device, uint32_t vocab_size, uint32_t n_states, uint32_t n_classes, const uint16_t* class_of, const uint32_t* next,
                                       uint32_t* bits_out) {
    const std::string what = "lmrs_op_automaton_masks: ";
    if (!bits_out) return fail(what + "NULL argument (bits_out)");
    if (automaton_check("lmrs_op_automaton_masks", AutomatonTables{vocab_size, n_states, n_classes, class_of, next, nullptr}, nullptr, true)) return -1;
    if (vocab_size > (1u << 24)) return fail(what + "vocab_size exceeds 2^24");
    if (op_begin(device)) return -1;
    const size_t V = vocab_size, W = (V + 31) / 32, cells = (size_t)n_states * n_classes;
    Scratch S;
    void *dc = S.get(V * 2), *dn = S.get(cells * 4), *db = S.get((size_t)n_states * W * 4);
    if (!dc || !dn || !db) return fail(what + "hipMalloc failed");
    HIP_OK(hipMemcpy(dc, class_of, V * 2, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dn, next, cells * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(db, 0xA5, (size_t)n_states * W * 4));                    // (a word the kernel failed to write shows)
    HIP_OK(launch_automaton_masks(static_cast<const uint16_t*>(dc), static_cast<const uint32_t*>(dn), (int)V, n_states, n_classes, static_cast<uint32_t*>(db), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(bits_out, db, (size_t)n_states * W * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_filter_rows on caller-supplied rows, in place (unit parity against the rule in numpy): row r is rows[r * ld .. r * ld + n), the floats between rows
// travel with them and come back as they went; a row with (0 or >= n, +inf) is handed to the launch as an unfiltered one (slot -1)
extern "C" int lmrs_op_filter_rows(int device, float* rows, size_t n_rows, size_t n, size_t ld, const uint32_t* top_k, const float* min_gap) {
    const std::string what = "lmrs_op_filter_rows: ";
    if (!rows || !top_k || !min_gap) return fail(what + "NULL argument");
    if (n_rows < 1 || n_rows > 65535) return fail(what + "n_rows = " + std::to_string(n_rows) + " is outside 1 .. 65535");
    if (n < 1 || n > ((size_t)1 << 24) || ld < n || ld > ((size_t)1 << 24)) return fail(what + "need 1 <= n <= ld <= 2^24");
    std::vector<FilterRow> of(n_rows);
    for (size_t r = 0; r < n_rows; ++r) {
        if (min_gap[r] != min_gap[r] || min_gap[r] < 0.0f) return fail(what + "row " + std::to_string(r) + ": min_gap is NaN or negative");
        const bool on = (top_k[r] != 0u && top_k[r] < n) || min_gap[r] < INFINITY;
        of[r] = FilterRow{on ? (int)r : -1, top_k[r], min_gap[r]};
    }
    if (op_begin(device)) return -1;
    Scratch S;
    const size_t bytes = n_rows * ld * 4;
    void *dl = S.get(bytes), *dof = S.get(n_rows * sizeof(FilterRow));
    if (!dl || !dof) return fail(what + "hipMalloc failed");
    HIP_OK(hipMemcpy(dl, rows, bytes, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dof, of.data(), n_rows * sizeof(FilterRow), hipMemcpyHostToDevice));
    HIP_OK(launch_filter_rows(static_cast<float*>(dl), (int)ld, (int)n, (int)n_rows, static_cast<const FilterRow*>(dof), nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(rows, dl, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// launch_topp_rows on caller-supplied rows (unit parity against lmrs_sampler_topp_pairs): result blocks as launch_sample_rows leaves them - {0, n0}, then
// the candidates - every row its own vector, in block 0 of its pair
static_assert(kToppRowsMax == (int)kWideBatchMax, "a vector per row of a wide batch");
extern "C" int lmrs_op_topp_rows(int device, size_t n_rows, size_t n, const void* cand, const uint32_t* n0, const float* top_p, const float* rnd,
                                 void* state, uint32_t* token, uint32_t* status) {
    const std::string what = "lmrs_op_topp_rows: ";
    if (!cand || !n0 || !top_p || !rnd || !state || !token || !status) return fail(what + "NULL argument");
    if (n_rows < 1 || n_rows > (size_t)kToppRowsMax) return fail(what + "n_rows = " + std::to_string(n_rows) + " is outside 1 .. " + std::to_string(kToppRowsMax));
    if (n < 2 || n > ((size_t)1 << 24)) return fail(what + "need 2 <= n <= 2^24");
    for (size_t r = 0; r < n_rows; ++r)
        if (n0[r] > n) return fail(what + "row " + std::to_string(r) + ": n0 = " + std::to_string(n0[r]) + " exceeds n = " + std::to_string(n));
    if (op_begin(device)) return -1;
    const size_t N = (size_t)topp_sort_n(n);
    Scratch S;
    void *dres = S.get(n_rows * (n + 1) * 8), *dtab = S.get(n_rows * sizeof(SampleRow)), *dof = S.get(n_rows * 4), *dst = S.get(n_rows * 2 * n * 8),
         *dwhich = S.get(n_rows * 4), *dext = S.get(n_rows * 8), *dkeys = S.get(n_rows * N * 8), *dstatus = S.get(n_rows * 4);
    if (!dres || !dtab || !dof || !dst || !dwhich || !dext || !dkeys || !dstatus) return fail("hipMalloc failed");
    std::vector<SampleRow> tab(n_rows); std::vector<uint32_t> of(n_rows), which(n_rows);
    for (size_t r = 0; r < n_rows; ++r) {
        tab[r] = SampleRow{1.0f, top_p[r], rnd[r]}; of[r] = (uint32_t)r;
        const unsigned long long head = (unsigned long long)n0[r] << 32;
        char* blk = static_cast<char*>(dres) + r * (n + 1) * 8;
        HIP_OK(hipMemcpy(blk, &head, 8, hipMemcpyHostToDevice));
        if (n0[r]) HIP_OK(hipMemcpy(blk + 8, static_cast<const char*>(cand) + r * n * 8, (size_t)n0[r] * 8, hipMemcpyHostToDevice));
        for (int blk2 = 0; blk2 < 2; ++blk2)
            HIP_OK(hipMemcpy(static_cast<char*>(dst) + (r * 2 + blk2) * n * 8, static_cast<const char*>(state) + r * n * 8, n * 8, hipMemcpyHostToDevice));
    }
    HIP_OK(hipMemset(dext, 0, n_rows * 8));
    HIP_OK(hipMemcpy(dtab, tab.data(), n_rows * sizeof(SampleRow), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dof, of.data(), n_rows * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dwhich, 0, n_rows * 4));
    HIP_OK(hipMemset(dstatus, 0xFF, n_rows * 4));
    HIP_OK(launch_topp_rows(ToppRowsArgs{static_cast<unsigned long long*>(dres), n + 1, static_cast<const SampleRow*>(dtab), static_cast<const uint32_t*>(dof),
                                         (int)n_rows, (int)n, static_cast<unsigned long long*>(dst), static_cast<uint32_t*>(dwhich), static_cast<uint32_t*>(dext),
                                         static_cast<unsigned long long*>(dkeys), (int)N, nullptr, nullptr, 0, static_cast<uint32_t*>(dstatus)}, nullptr));
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(which.data(), dwhich, n_rows * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(status, dstatus, n_rows * 4, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < n_rows; ++r) {
        if (status[r] > 1u || (which[r] & 1u) != (status[r] ^ 1u)) return fail(what + "row " + std::to_string(r) + ": the device left no result");
        unsigned long long head = 0;
        HIP_OK(hipMemcpy(&head, static_cast<const char*>(dres) + r * (n + 1) * 8, 8, hipMemcpyDeviceToHost));
        token[r] = status[r] ? 0u : (uint32_t)head;
        HIP_OK(hipMemcpy(static_cast<char*>(state) + r * n * 8, static_cast<const char*>(dst) + (r * 2 + (which[r] & 1u)) * n * 8, n * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

// measurement: launch_topp_rows on n_rows rows of n0 candidates each (scattered probabilities, index order) over vectors that carry the steps before;
// *us = the device time of all its launches (HIP events on each dispatch, summed) per run, the mean of iters runs after one warm-up; *launches: how many
extern "C" int lmrs_bench_topp_rows(int device, size_t n_rows, size_t n, size_t n0, int iters, double* us, int* launches) {
    if (!us || iters < 1 || n_rows < 1 || n_rows > (size_t)kToppRowsMax || n < 2 || n > ((size_t)1 << 24) || n0 < 1 || n0 > n) return fail("lmrs_bench_topp_rows: bad argument");
    if (op_begin(device)) return -1;
    const size_t N = (size_t)topp_sort_n(n);
    const int K = topp_launches((int)N);
    Scratch S;
    void *dres = S.get(n_rows * (n + 1) * 8), *dtab = S.get(n_rows * sizeof(SampleRow)), *dof = S.get(n_rows * 4), *dst = S.get(n_rows * 2 * n * 8),
         *dwhich = S.get(n_rows * 4), *dext = S.get(n_rows * 8), *dkeys = S.get(n_rows * N * 8);
    if (!dres || !dtab || !dof || !dst || !dwhich || !dext || !dkeys) return fail("hipMalloc failed");
    std::vector<unsigned long long> blk(n0 + 1);
    blk[0] = (unsigned long long)n0 << 32;
    for (size_t i = 0; i < n0; ++i) {
        const float p = (float)(1 + (i * 2654435761ull) % 4093) / (4096.0f * (float)n0);
        uint32_t bits; memcpy(&bits, &p, 4);
        blk[1 + i] = ((unsigned long long)(uint32_t)(i * (n / n0)) << 32) | bits;
    }
    std::vector<SampleRow> tab(n_rows, SampleRow{1.0f, 0.9f, 0.5f}); std::vector<uint32_t> of(n_rows);
    for (size_t r = 0; r < n_rows; ++r) { of[r] = (uint32_t)r; HIP_OK(hipMemcpy(static_cast<char*>(dres) + r * (n + 1) * 8, blk.data(), (n0 + 1) * 8, hipMemcpyHostToDevice)); }
    HIP_OK(hipMemcpy(dtab, tab.data(), n_rows * sizeof(SampleRow), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dof, of.data(), n_rows * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dwhich, 0, n_rows * 4));
    HIP_OK(hipMemset(dst, 0, n_rows * 2 * n * 8));
    HIP_OK(hipMemset(dext, 0, n_rows * 8));
    const ToppRowsArgs a{static_cast<unsigned long long*>(dres), n + 1, static_cast<const SampleRow*>(dtab), static_cast<const uint32_t*>(dof), (int)n_rows, (int)n,
                         static_cast<unsigned long long*>(dst), static_cast<uint32_t*>(dwhich), static_cast<uint32_t*>(dext), static_cast<unsigned long long*>(dkeys), (int)N, nullptr,
                         nullptr, 0, nullptr};
    std::vector<hipEvent_t> ev(2 * (size_t)K);
    for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    *us = 0.0;
    int rc = 0;
    for (int it = -1; it < iters && !rc; ++it) {
        set_launch_event_pool(ev.data(), K);
        const hipError_t le = launch_topp_rows(a, nullptr);
        const int used = launch_event_pool_used();
        set_launch_event_pool(nullptr, 0);
        if (le != hipSuccess || hipDeviceSynchronize() != hipSuccess || used != K) { rc = fail("lmrs_bench_topp_rows: the launches failed"); break; }
        for (int k = 0; k < K && it >= 0; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) != hipSuccess) { rc = fail("hipEventElapsedTime failed"); break; } *us += (double)ms * 1e3 / iters; }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc) return -1;
    if (launches) *launches = K;
    return 0;
}

// measurement: the six launches of launch_sample_rows on n_rows rows of n equal logits, every row a sample_mult row whose random number no cdf reaches - both
// chains walk all n terms.  us6[k] = the device time of launch k (HIP events on the dispatch itself), summed over iters runs after one warm-up;
// *clock_mhz = the device's nominal shader clock
extern "C" int lmrs_bench_sample_rows(int device, size_t n_rows, size_t n, int iters, double* us6, double* clock_mhz) {
    if (!us6 || iters < 1 || n_rows < 1 || n_rows > (size_t)kSampleRowsMax || n < 1 || n > (size_t)0x7FFFFFFF / 2) return fail("lmrs_bench_sample_rows: bad argument");
    if (op_begin(device)) return -1;
    Scratch S;
    void *dl = S.get(n_rows * n * 4), *dt = S.get(n_rows * sizeof(SampleRow)), *ds = S.get(sample_scratch_floats(n_rows) * 4), *dout = S.get(n_rows * (n + 1) * 8);
    if (!dl || !dt || !ds || !dout) return fail("hipMalloc failed");
    std::vector<SampleRow> tab(n_rows, SampleRow{0.8f, 1.0f, 2.0f});
    HIP_OK(hipMemcpy(dt, tab.data(), n_rows * sizeof(SampleRow), hipMemcpyHostToDevice));
    const SampleRowsArgs a = sample_rows_args(static_cast<float*>(dl), (int)n_rows, (int)n, (int)n, static_cast<const SampleRow*>(dt), nullptr,
                                              static_cast<float*>(ds), static_cast<unsigned long long*>(dout));
    hipEvent_t ev[12]; int tags[6];
    for (auto& e : ev) HIP_OK(hipEventCreate(&e));
    for (int k = 0; k < 6; ++k) us6[k] = 0.0;
    int rc = 0;
    for (int it = -1; it < iters && !rc; ++it) {
        if (hipMemset(dl, 0, n_rows * n * 4) != hipSuccess) { rc = fail("hipMemset failed"); break; }
        set_launch_event_pool(ev, 6, tags);
        const hipError_t le = launch_sample_rows(a, nullptr);
        const int used = launch_event_pool_used();
        set_launch_event_pool(nullptr, 0);
        if (le != hipSuccess || hipDeviceSynchronize() != hipSuccess || used != 6) { rc = fail("lmrs_bench_sample_rows: the launches failed"); break; }
        for (int k = 0; k < 6 && it >= 0; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]) != hipSuccess) { rc = fail("hipEventElapsedTime failed"); break; } us6[k] += (double)ms * 1e3; }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    if (rc) return -1;
    int khz = 0;
    HIP_OK(hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device));
    if (clock_mhz) *clock_mhz = khz / 1000.0;
    return 0;
}

// launch_topk_rows on one caller-supplied row: the ordering rule on the cases whole models do not reach (NaNs, signed zeros, rows of equal values,
// k = n).  Columns [written, n) are never uploaded - the device row holds NaN patterns there - and count as 0.0.
extern "C" int lmrs_op_topk(int device, const float* logits, size_t n, size_t written, uint32_t k, uint32_t* idx, float* val) {
    if (!logits || !idx || !val) return fail("NULL argument");
    if (n == 0 || n > (size_t)0x7FFFFFFF || written > n) return fail("lmrs_op_topk: need 1 <= n < 2^31 and written <= n");
    if (topk_check_k(k, (uint32_t)n)) return -1;
    if (op_begin(device)) return -1;
    Scratch S; const size_t C = (size_t)score_chunks((int)n);
    void *dl = S.get(n * 4), *dc = S.get(C * k * 8), *di = S.get((size_t)k * 4), *dv = S.get((size_t)k * 4);
    if (!dl || !dc || !di || !dv) return fail("hipMalloc failed");
    HIP_OK(hipMemset(dl, 0xFF, n * 4));
    HIP_OK(hipMemcpy(dl, logits, written * 4, hipMemcpyHostToDevice));
    TopkArgs t{static_cast<float*>(dl), (int)n, (int)written, (int)n, 1, (int)k, nullptr, 0, nullptr, static_cast<unsigned long long*>(dc), nullptr,
               static_cast<uint32_t*>(di), static_cast<float*>(dv), nullptr};
    HIP_OK(launch_topk_rows(t, nullptr));
    HIP_OK(hipMemcpy(idx, di, (size_t)k * 4, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(val, dv, (size_t)k * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lmrs_op_tanh_cast(int device, float* y, const float* x, size_t n, double c) {
    if (op_begin(device)) return -1;
    if (!x || !y) return fail("NULL argument");
    Scratch S; void *dx = S.get(n * 4), *dy = S.get(n * 4);
    if (!dy) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
    HIP_OK(launch_tanh_cast(static_cast<float*>(dx), static_cast<float*>(dy), n, c, nullptr));
    HIP_OK(hipMemcpy(y, dy, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int lmrs_op_expf(int device, float* y, const float* x, size_t n) {
    if (op_begin(device)) return -1;
    Scratch S; void *dx = S.get(n * 4), *dy = S.get(n * 4);
    if (!dy) return fail("hipMalloc failed");
    HIP_OK(hipMemcpy(dx, x, n * 4, hipMemcpyHostToDevice));
    HIP_OK(launch_expf(static_cast<float*>(dx), static_cast<float*>(dy), n, nullptr));
    HIP_OK(hipMemcpy(y, dy, n * 4, hipMemcpyDeviceToHost));
    return 0;
}


// ==================================================================================================
// CLIP vision tower (reference src/vision.rs): VisionTransformer::new :99-243, forward :244-577.  Q8_0 (tuned), Q4_0 and f32 sections.
// ==================================================================================================
struct VisLayer {
    float *ln1 = nullptr, *ln1_b = nullptr, *ln2 = nullptr, *ln2_b = nullptr, *bqkv = nullptr, *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
    char *wqkv = nullptr, *wo = nullptr, *w1 = nullptr, *w2 = nullptr; float *sqkv = nullptr, *so = nullptr, *s1 = nullptr, *s2 = nullptr;   // weights: int8 / packed nibbles / f32; scales (quantised only)
    float *sqkvT = nullptr, *soT = nullptr, *s1T = nullptr, *s2T = nullptr;            // the scales transposed, [group][row] (made at the first forward: GemmArgs::ws_ld)
};
struct lmrs_vision {
    int device = 0; hipStream_t stream = nullptr;
    uint32_t dim = 0, hidden = 0, n_layers = 0, n_heads = 0, head_size = 0, patch = 0, image = 0, gs = 0; float eps = 0;
    int qt = LMRS_Q8_0;                            // q_type of the section: Q8_0, Q4_0 or None (f32)
    bool no_scales_t = false;                      // the transposed scale copies could not be allocated: row-major scales stay in use
    Switches sw;                                   // the environment switches, read at create (vis_no_stray)
    float *class_emb = nullptr, *patch_emb = nullptr, *pos_emb = nullptr, *pre_ln = nullptr, *pre_ln_b = nullptr;
    std::vector<VisLayer> layers;
    std::vector<DevBuf<char>> owned;               // the weights' blocks (the pointers above and the layers' are views of them)
    // work buffers, grown on demand (alloc_all; cap_tok != 0: the set stands)
    size_t cap_tok = 0;
    DevBuf<float> pix, X, E, QKV, AO, H, scratch, xs; DevBuf<int8_t> xq;
};

namespace {
template <class T> T* vis_dev(lmrs_vision* v, const void* src, size_t bytes) {
    DevBuf<char> d;
    if (!d.alloc(bytes)) return nullptr;
    void* p = d.get();
    v->owned.push_back(std::move(d));
    if (src && hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return static_cast<T*>(p);
}
uint32_t rd32(const uint8_t* p) { uint32_t x; memcpy(&x, p, 4); return x; }
}  // namespace

extern "C" void lmrs_vision_destroy(lmrs_vision* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

extern "C" int lmrs_vision_create(const uint8_t* sec, size_t len, int device, lmrs_vision** out, size_t* bytes_consumed) {
    if (!sec || !out) return fail("NULL argument");
    if (op_begin(device)) return -1;
    if (len < 128) return fail("vision section shorter than its 128-byte header");
    lmrs_vision* v = new lmrs_vision();
    v->sw = read_switches();
    v->device = device;
    v->dim = rd32(sec); v->hidden = rd32(sec + 4); v->n_layers = rd32(sec + 8); v->n_heads = rd32(sec + 12); v->head_size = rd32(sec + 16);
    memcpy(&v->eps, sec + 20, 4); v->patch = rd32(sec + 24); v->image = rd32(sec + 28);
    const uint8_t q_type = sec[32]; v->gs = rd32(sec + 33);
    auto bad = [&](const char* m) { lmrs_vision_destroy(v); return fail(m); };
    if (q_type != LMRS_Q8_0 && q_type != LMRS_Q4_0 && q_type != LMRS_Q_NONE) return bad("vision section: unknown q_type");
    if (q_type != LMRS_Q_NONE && v->gs != 128) return bad("the vision tower is built for quantised sections with group size 128 (what the exporter writes)");
    v->qt = q_type;
    // the reference hard-codes 577 positions (vision.rs:117); the kernels are built for CLIP ViT-L/14-336 geometry
    if (v->dim != 1024 || v->head_size != 64 || v->n_heads * v->head_size != v->dim || v->patch == 0 || (v->image / v->patch) * (v->image / v->patch) != 576 ||
        v->hidden % 256 || v->hidden != 4096 || v->n_layers < 2)
        return bad("unsupported vision geometry (built for CLIP ViT-L/14-336: dim 1024, 16 heads of 64, 576 patches, hidden 4096)");
    const size_t dim = v->dim, L = v->n_layers, hid = v->hidden, kdim = 3ull * v->patch * v->patch;
    // bytes of a weight tensor's values / group scales: int8, packed nibbles (init_param_quant, transformer.rs:24-48) or plain f32
    auto qb = [&](size_t cnt) { return q_type == LMRS_Q_NONE ? cnt * 4 : (q_type == LMRS_Q4_0 ? cnt / 2 : cnt); };
    auto sb = [&](size_t cnt) { return q_type == LMRS_Q_NONE ? (size_t)0 : cnt / 128 * 4; };
    const size_t need = 128 + 4 * (dim + dim * kdim + dim * 577 + 8 * L * dim + L * hid + L * dim + 2 * dim) +
                        L * (4 * (qb(dim * dim) + sb(dim * dim)) + 2 * (qb(dim * hid) + sb(dim * hid)));
    if (len < need) return bad("vision section truncated");
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) return bad("hipStreamCreate failed");
    size_t off = 128;
    auto f32v = [&](size_t count) { const uint8_t* p = sec + off; off += count * 4; return p; };
    v->class_emb = vis_dev<float>(v, f32v(dim), dim * 4);
    v->patch_emb = vis_dev<float>(v, f32v(dim * kdim), dim * kdim * 4);
    v->pos_emb = vis_dev<float>(v, f32v(dim * 577), dim * 577 * 4);
    v->layers.resize(L);
    const uint8_t *ln1 = f32v(L * dim), *ln1b = f32v(L * dim), *ln2 = f32v(L * dim), *ln2b = f32v(L * dim);
    // weight tensors: per layer {values [rows*cols], f32 scales [rows*cols/128] (quantised only)}, then the bias block of all layers
    struct QT { const uint8_t* q[64]; const uint8_t* s[64]; const uint8_t* bias; };
    if (L > 64) return bad("too many vision layers");
    auto quant = [&](size_t rows, size_t cols, size_t bias_len, QT& t) {
        for (size_t l = 0; l < L; ++l) { t.q[l] = sec + off; off += qb(rows * cols); t.s[l] = sec + off; off += sb(rows * cols); }
        t.bias = sec + off; off += L * bias_len * 4;
    };
    QT tq, tk, tv, to, t1, t2;
    quant(dim, dim, dim, tq); quant(dim, dim, dim, tk); quant(dim, dim, dim, tv); quant(dim, dim, dim, to);
    quant(hid, dim, hid, t1); quant(dim, hid, dim, t2);
    v->pre_ln = vis_dev<float>(v, f32v(dim), dim * 4);
    v->pre_ln_b = vis_dev<float>(v, f32v(dim), dim * 4);
    if (off != need) return bad("vision layout arithmetic");
    const size_t qdd = qb(dim * dim), sdd = sb(dim * dim), qdh = qb(dim * hid), sdh = sb(dim * hid);
    for (size_t l = 0; l < L; ++l) {
        VisLayer& Y = v->layers[l];
        Y.ln1 = vis_dev<float>(v, ln1 + l * dim * 4, dim * 4); Y.ln1_b = vis_dev<float>(v, ln1b + l * dim * 4, dim * 4);
        Y.ln2 = vis_dev<float>(v, ln2 + l * dim * 4, dim * 4); Y.ln2_b = vis_dev<float>(v, ln2b + l * dim * 4, dim * 4);
        // q | k | v rows concatenated: one GEMM
        Y.wqkv = vis_dev<char>(v, nullptr, 3 * qdd); Y.sqkv = vis_dev<float>(v, nullptr, 3 * sdd); Y.bqkv = vis_dev<float>(v, nullptr, 3 * dim * 4);
        if (!Y.wqkv || !Y.sqkv || !Y.bqkv) return bad("hipMalloc failed");
        const QT* three[3] = {&tq, &tk, &tv};
        for (int w = 0; w < 3; ++w) {
            if (hipMemcpy(Y.wqkv + (size_t)w * qdd, three[w]->q[l], qdd, hipMemcpyHostToDevice) != hipSuccess ||
                (sdd && hipMemcpy(reinterpret_cast<char*>(Y.sqkv) + (size_t)w * sdd, three[w]->s[l], sdd, hipMemcpyHostToDevice) != hipSuccess) ||
                hipMemcpy(Y.bqkv + (size_t)w * dim, three[w]->bias + l * dim * 4, dim * 4, hipMemcpyHostToDevice) != hipSuccess)
                return bad("upload of the vision weights failed");
        }
        Y.wo = vis_dev<char>(v, to.q[l], qdd); Y.so = vis_dev<float>(v, to.s[l], sdd); Y.bo = vis_dev<float>(v, to.bias + l * dim * 4, dim * 4);
        Y.w1 = vis_dev<char>(v, t1.q[l], qdh); Y.s1 = vis_dev<float>(v, t1.s[l], sdh); Y.b1 = vis_dev<float>(v, t1.bias + l * hid * 4, hid * 4);
        Y.w2 = vis_dev<char>(v, t2.q[l], qdh); Y.s2 = vis_dev<float>(v, t2.s[l], sdh); Y.b2 = vis_dev<float>(v, t2.bias + l * dim * 4, dim * 4);
        if (!Y.ln1 || !Y.ln1_b || !Y.ln2 || !Y.ln2_b || !Y.wo || !Y.so || !Y.bo || !Y.w1 || !Y.s1 || !Y.b1 || !Y.w2 || !Y.s2 || !Y.b2) return bad("hipMalloc failed");
    }
    if (!v->class_emb || !v->patch_emb || !v->pos_emb || !v->pre_ln || !v->pre_ln_b) return bad("hipMalloc failed");
    if (bytes_consumed) *bytes_consumed = off;
    *out = v;
    return 0;
}

static int vis_reserve(lmrs_vision* v, size_t n_tok, uint32_t num_crops) {
    if (n_tok <= v->cap_tok) return 0;
    v->cap_tok = 0;
    const size_t dim = v->dim, hid = v->hidden;
    if (!alloc_all({{v->pix, (size_t)num_crops * 3 * v->image * v->image}, {v->X, n_tok * dim}, {v->E, n_tok * dim}, {v->QKV, n_tok * dim * 3}, {v->AO, n_tok * dim}, {v->H, n_tok * hid},
                    {v->scratch, vis_attention_scratch_floats((int)num_crops, (int)v->n_heads, 577)}, {v->xq, n_tok * hid}, {v->xs, n_tok * (hid / 128)}}))
        return alloc_failed("vision work buffers: hipMalloc");
    v->cap_tok = n_tok;
    return 0;
}

// VisionTransformer::forward (vision.rs:244-577): pixel_values = num_crops * 3 * image^2 floats cut into patches
// (processor.rs view_as_patches); out = num_crops * 576 * dim floats (CLS dropped); *new_shape = 576 * dim.
extern "C" int lmrs_vision_forward(lmrs_vision* v, const float* pixel_values, uint32_t num_crops, float* out, uint32_t* new_shape) {
    if (!v || !pixel_values || !out) return fail("NULL argument");
    if (num_crops == 0 || num_crops > 64) return fail("num_crops out of range");
    HIP_OK(hipSetDevice(v->device));
    const int dim = (int)v->dim, hid = (int)v->hidden, T = 577, n_tok = (int)num_crops * T;
    if (vis_reserve(v, (size_t)n_tok, num_crops)) return -1;
    hipStream_t s = v->stream;
    const size_t img = 3ull * v->image * v->image;
    HIP_OK(hipMemcpyAsync(v->pix, pixel_values, (size_t)num_crops * img * 4, hipMemcpyHostToDevice, s));
    VisPatchArgs pa{v->pix, v->patch_emb, v->class_emb, v->pos_emb, v->E, dim, 576, (int)(3 * v->patch * v->patch)};
    HIP_OK(launch_vis_patch_embed(pa, (int)num_crops, s));
    HIP_OK(launch_vis_layernorm(v->E, v->pre_ln, v->pre_ln_b, v->eps, dim, n_tok, v->X, nullptr, nullptr, s));     // input layernorm (:293-301)
    // One projection of the whole batch: quantise the rows with the section's quantiser (Q8_0: fused into the layernorm where
    // there is one; Q4_0: rows_prologue_kernel's Q4 flavour) and run the int8-MFMA GEMM, or the f32 matmul kernel (q_type None).
    // src_f32: the rows [n_tok][n] (for Q8_0 with pre_quantised = true they are already in xq / xs).
    // scale layouts (round 6): the ring GEMMs of a batch of >= 48 rows take TRANSPOSED scales - the layers' copies are made here, once; the activation scales
    // are written that way by the layernorm / quantise rows (leading dimension n_tok)
    if (v->qt == LMRS_Q8_0 && !v->layers.empty() && !v->layers[0].sqkvT && !v->no_scales_t) {      // (Q4_0 sections run the direct kernels: row-major scales)
        bool ok = true;
        auto tr = [&](const float* src, int rows, int groups) -> float* {
            float* d = ok ? vis_dev<float>(v, nullptr, (size_t)rows * groups * 4) : nullptr;
            if (!d) { (void)hipGetLastError(); ok = false; return nullptr; }
            if (launch_transpose_scales(src, rows, groups, d, s) != hipSuccess) ok = false;
            return d;
        };
        for (VisLayer& Y : v->layers) { Y.sqkvT = tr(Y.sqkv, 3 * dim, dim / 128); Y.soT = tr(Y.so, dim, dim / 128); Y.s1T = tr(Y.s1, hid, dim / 128); Y.s2T = tr(Y.s2, dim, hid / 128); }
        if (!ok) { for (VisLayer& Y : v->layers) Y.sqkvT = Y.soT = Y.s1T = Y.s2T = nullptr; v->no_scales_t = true; }
    }
    const bool trs = n_tok >= 48 && v->qt == LMRS_Q8_0 && v->layers[0].sqkvT != nullptr;
    const int xld = trs ? n_tok : 0;
    auto project = [&](const float* src_f32, bool pre_quantised, const char* w, const float* ws, const float* wsT, int n, int o, GemmArgs g, int epi) -> int {
        g.wq = w; g.ws = ws; g.n = n; g.o = o; g.n_tok = n_tok;
        if (v->qt == LMRS_Q_NONE) { g.xf = src_f32; HIP_OK(launch_matmul_f32_rows(g, epi, s)); return 0; }
        if (!pre_quantised) HIP_OK(launch_rows_prologue(const_cast<float*>(src_f32), nullptr, nullptr, nullptr, 0.f, 0, 0, v->qt == LMRS_Q4_0, n, n_tok, v->xq, v->xs, s, xld));
        g.xq = v->xq; g.xs = v->xs; g.q4 = v->qt == LMRS_Q4_0;
        if (trs) { g.ws = wsT; g.ws_ld = o; g.xs_ld = xld; }
        HIP_OK(launch_gemm_q8(g, epi, s));
        return 0;
    };
    const bool q8 = v->qt == LMRS_Q8_0;
    for (uint32_t l = 0; l + 1 < v->n_layers; ++l) {                      // the penultimate layer's output is used (:303)
        const VisLayer& Y = v->layers[l];
        // layernorm 1 (Q8_0: quantised in the same launch; otherwise f32 rows into AO, which is free until the attention writes it)
        HIP_OK(launch_vis_layernorm(v->X, Y.ln1, Y.ln1_b, v->eps, dim, n_tok, q8 ? nullptr : v->AO, v->xq, v->xs, s, xld));
        GemmArgs g{};
        g.out = v->QKV; g.bias = Y.bqkv; g.att_dim = dim; g.qscale = sqrtf((float)v->head_size);
        if (project(v->AO, q8, Y.wqkv, Y.sqkv, Y.sqkvT, dim, 3 * dim, g, EPI_VQKV)) return -1;
        HIP_OK(launch_vis_attention(v->QKV, v->AO, v->scratch, (int)num_crops, (int)v->n_heads, T, dim, !v->sw.vis_no_stray, s));
        g = GemmArgs{}; g.out = v->E; g.bias = Y.bo; g.resid = v->X;
        if (project(v->AO, false, Y.wo, Y.so, Y.soT, dim, dim, g, EPI_BIAS_RESID)) return -1;
        HIP_OK(launch_vis_layernorm(v->E, Y.ln2, Y.ln2_b, v->eps, dim, n_tok, q8 ? nullptr : v->AO, v->xq, v->xs, s, xld));
        g = GemmArgs{}; g.out = v->H; g.bias = Y.b1;
        if (project(v->AO, q8, Y.w1, Y.s1, Y.s1T, dim, hid, g, EPI_BIAS_QGELU)) return -1;
        g = GemmArgs{}; g.out = v->X; g.bias = Y.b2; g.resid = v->E;
        if (project(v->H, false, Y.w2, Y.s2, Y.s2T, hid, dim, g, EPI_BIAS_RESID)) return -1;
    }
    for (uint32_t c = 0; c < num_crops; ++c)                               // drop the CLS embedding (:571-579)
        HIP_OK(hipMemcpyAsync(out + (size_t)c * 576 * dim, v->X + ((size_t)c * T + 1) * dim, (size_t)576 * dim * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (new_shape) *new_shape = 576u * (uint32_t)dim;
    return 0;
}


// ==================================================================================================
// PHI3VProcessor (reference src/processor.rs): new :168-232, forward :234-342.  Q8_0 sections.
// The HD transform (reshape_hd_patches_2x2merge :377-418, add_image_newline :480-484) is data movement and runs on the host
// where the tower's output already is; the projector MLP runs as two int8 matrix-core GEMMs over all embeddings.
// ==================================================================================================
struct lmrs_processor {
    int device = 0; hipStream_t stream = nullptr;
    uint32_t hidden = 0, text = 0; int qt = LMRS_Q8_0;       // q_type of the section: Q8_0, Q4_0 or None (f32)
    std::vector<float> glb_gn, sub_gn;
    DevBuf<char> p0, p1; DevBuf<float> s0, s1, b0, b1;
    size_t cap = 0; DevBuf<float> emb, hid, outd, xs; DevBuf<int8_t> xq;        // work buffers for cap embeddings (alloc_all)
};

extern "C" void lmrs_processor_destroy(lmrs_processor* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
}

extern "C" int lmrs_processor_create(const uint8_t* sec, size_t len, int device, lmrs_processor** out, size_t* bytes_consumed) {
    if (!sec || !out) return fail("NULL argument");
    if (op_begin(device)) return -1;
    if (len < 128) return fail("processor section shorter than its 128-byte header");
    lmrs_processor* p = new lmrs_processor();
    p->device = device; p->hidden = rd32(sec); p->text = rd32(sec + 4);
    const uint8_t q_type = sec[8]; const uint32_t gs = rd32(sec + 9);
    auto bad = [&](const char* m) { lmrs_processor_destroy(p); return fail(m); };
    if (q_type != LMRS_Q8_0 && q_type != LMRS_Q4_0 && q_type != LMRS_Q_NONE) return bad("processor section: unknown q_type");
    if (q_type != LMRS_Q_NONE && gs != 128) return bad("the image projector is built for quantised sections with group size 128 (what the exporter writes)");
    p->qt = q_type;
    // reshape_hd_patches_2x2merge hard-codes C = 1024 (processor.rs:378): hidden_dim = 4 * 1024
    if (p->hidden != 4096 || !rows_prologue_supported((int)p->text) || p->text % 16) return bad("unsupported projector geometry (4096 -> text_dim in {2048, 3072})");
    const size_t H = p->hidden, Tt = p->text;
    auto qb = [&](size_t cnt) { return q_type == LMRS_Q_NONE ? cnt * 4 : (q_type == LMRS_Q4_0 ? cnt / 2 : cnt); };
    auto sb = [&](size_t cnt) { return q_type == LMRS_Q_NONE ? (size_t)0 : cnt / 128 * 4; };
    const size_t need = 128 + 4 * (2 * H + 2 * Tt) + qb(Tt * H) + sb(Tt * H) + qb(Tt * Tt) + sb(Tt * Tt);
    if (len < need) return bad("processor section truncated");
    if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) return bad("hipStreamCreate failed");
    size_t off = 128;
    p->glb_gn.assign(reinterpret_cast<const float*>(sec + off), reinterpret_cast<const float*>(sec + off) + H); off += H * 4;
    p->sub_gn.assign(reinterpret_cast<const float*>(sec + off), reinterpret_cast<const float*>(sec + off) + H); off += H * 4;
    auto up = [&](auto& dst, size_t bytes) {
        if (!dst.alloc(bytes / sizeof(*dst.get()))) return false;
        const bool ok = !bytes || hipMemcpy(dst, sec + off, bytes, hipMemcpyHostToDevice) == hipSuccess; off += bytes; return ok; };
    if (!up(p->p0, qb(Tt * H)) || !up(p->s0, sb(Tt * H)) || !up(p->p1, qb(Tt * Tt)) || !up(p->s1, sb(Tt * Tt)) || !up(p->b0, Tt * 4) || !up(p->b1, Tt * 4))
        return bad("hipMalloc / upload failed");
    if (bytes_consumed) *bytes_consumed = off;
    *out = p;
    return 0;
}

// reshape_hd_patches_2x2merge (processor.rs:377-418) followed by add_image_newline (:480-484): rows of 4 * 1024 floats
static void hd_merge_with_newlines(const float* feat, size_t n_floats, size_t h_crop, size_t w_crop, const float* sep, std::vector<float>& res) {
    const size_t C = 1024, H = 24, Lp = H * H, out_c = 4 * C;
    const size_t n = n_floats / (Lp * C), num_images = n / (h_crop * w_crop), out_h = h_crop * H / 2, out_w = w_crop * H / 2;
    std::vector<float> merged(num_images * out_h * out_w * out_c);
    for (size_t img = 0; img < num_images; ++img)
        for (size_t hc = 0; hc < h_crop; ++hc)
            for (size_t wc = 0; wc < w_crop; ++wc) {
                const size_t patch_idx = img * h_crop * w_crop + hc * w_crop + wc;
                for (size_t i = 0; i < H / 2; ++i)
                    for (size_t j = 0; j < H / 2; ++j) {
                        float* dst = merged.data() + ((img * out_h + hc * H / 2 + i) * out_w + wc * H / 2 + j) * out_c;
                        for (size_t di = 0; di < 2; ++di)
                            for (size_t dj = 0; dj < 2; ++dj)
                                memcpy(dst + (di * 2 + dj) * C, feat + patch_idx * Lp * C + ((i * 2 + di) * H + (j * 2 + dj)) * C, C * 4);
                    }
            }
    const size_t total = num_images * out_h * out_w;
    res.clear(); res.reserve((total + out_h) * out_c);
    size_t src = 0;
    for (size_t i = 0; i < out_h; ++i) {                                       // a separator after every row of out_w embeddings
        res.insert(res.end(), merged.begin() + src * out_c, merged.begin() + (src + out_w) * out_c); src += out_w;
        res.insert(res.end(), sep, sep + out_c);
    }
    res.insert(res.end(), merged.begin() + src * out_c, merged.begin() + total * out_c);
}

// The projector's input rows (processor.rs:240-254): sub-image features, glb_GN, global features - H floats per row
static void hd_embeddings(const float* out_patches, size_t total_floats, size_t new_shape, size_t w_crop, size_t h_crop,
                          const float* glb_gn, const float* sub_gn, size_t H, std::vector<float>& emb) {
    std::vector<float> glob, sub;
    hd_merge_with_newlines(out_patches, new_shape, 1, 1, sub_gn, glob);
    hd_merge_with_newlines(out_patches + new_shape, total_floats - new_shape, h_crop, w_crop, sub_gn, sub);
    emb.clear(); emb.reserve(sub.size() + H + glob.size());
    emb.insert(emb.end(), sub.begin(), sub.end()); emb.insert(emb.end(), glb_gn, glb_gn + H); emb.insert(emb.end(), glob.begin(), glob.end());
}

// Host-only verification aid (no device needed): exactly the rows lmrs_processor_forward feeds to the projector, for given
// separators.  out: n_embeds * 4096 floats; *n_embeds = (h_crop*12)*(w_crop*12+1) + 12*13 + 1.
extern "C" int lmrs_processor_hd_transform(const float* out_patches, uint32_t total_floats, uint32_t new_shape, uint32_t w_crop, uint32_t h_crop,
                                           const float* glb_gn, const float* sub_gn, float* out, uint32_t* n_embeds) {
    if (!out_patches || !glb_gn || !sub_gn || !out) return fail("NULL argument");
    if (new_shape != 576u * 1024u || w_crop == 0 || h_crop == 0 || (size_t)total_floats != (size_t)new_shape * (1 + (size_t)w_crop * h_crop))
        return fail("processor: out_patches must hold the global crop and h_crop * w_crop sub-images of 576 x 1024 floats");
    std::vector<float> emb;
    hd_embeddings(out_patches, total_floats, new_shape, w_crop, h_crop, glb_gn, sub_gn, 4096, emb);
    memcpy(out, emb.data(), emb.size() * 4);
    if (n_embeds) *n_embeds = (uint32_t)(emb.size() / 4096);
    return 0;
}

// PHI3VProcessor::forward (processor.rs:234-342).  out_patches: the tower's output (total_floats floats: the global crop first,
// new_shape floats, then the h_crop x w_crop sub-images); out: num_embeds * text_dim floats; *n_embeds = number of embeddings.
extern "C" int lmrs_processor_forward(lmrs_processor* p, const float* out_patches, uint32_t total_floats, uint32_t new_shape, uint32_t patch_side,
                                      uint32_t w_crop, uint32_t h_crop, float* out, uint32_t* n_embeds) {
    if (!p || !out_patches || !out) return fail("NULL argument");
    if (patch_side != 12 || new_shape != 576u * 1024u || w_crop == 0 || h_crop == 0 || (size_t)total_floats != (size_t)new_shape * (1 + (size_t)w_crop * h_crop))
        return fail("processor: out_patches must hold the global crop and h_crop * w_crop sub-images of 576 x 1024 floats (patch_side 12)");
    HIP_OK(hipSetDevice(p->device));
    const size_t H = p->hidden, Tt = p->text;
    std::vector<float> emb;
    hd_embeddings(out_patches, total_floats, new_shape, w_crop, h_crop, p->glb_gn.data(), p->sub_gn.data(), H, emb);
    const size_t ne = emb.size() / H;
    if (ne != (size_t)(h_crop * patch_side) * (w_crop * patch_side + 1) + (size_t)patch_side * (patch_side + 1) + 1) return fail("processor: embedding count");
    if (ne > p->cap) {
        p->cap = 0;
        if (!alloc_all({{p->emb, ne * H}, {p->hid, ne * Tt}, {p->outd, ne * Tt}, {p->xq, ne * H}, {p->xs, ne * (H / 128)}})) return alloc_failed("projector work buffers: hipMalloc");
        p->cap = ne;
    }
    hipStream_t s = p->stream;
    HIP_OK(hipMemcpyAsync(p->emb, emb.data(), ne * H * 4, hipMemcpyHostToDevice, s));
    // the two matmuls of every row (processor.rs:262-336): the section's quantiser + the int8-MFMA GEMM, or the f32 matmul kernel
    auto project = [&](float* src, const char* w, const float* ws, size_t n, float* dst, const float* bias, int epi) -> int {
        GemmArgs g{};
        g.wq = w; g.ws = ws; g.n = (int)n; g.o = (int)Tt; g.n_tok = (int)ne; g.out = dst; g.bias = bias;
        if (p->qt == LMRS_Q_NONE) { g.xf = src; HIP_OK(launch_matmul_f32_rows(g, epi, s)); return 0; }
        HIP_OK(launch_rows_prologue(src, nullptr, nullptr, nullptr, 0.f, 0, 0, p->qt == LMRS_Q4_0, (int)n, (int)ne, p->xq, p->xs, s));
        g.xq = p->xq; g.xs = p->xs; g.q4 = p->qt == LMRS_Q4_0;
        HIP_OK(launch_gemm_q8(g, epi, s));
        return 0;
    };
    if (project(p->emb, p->p0, p->s0, H, p->hid, p->b0, EPI_BIAS_GELU)) return -1;
    if (project(p->hid, p->p1, p->s1, Tt, p->outd, p->b1, EPI_BIAS)) return -1;
    HIP_OK(hipMemcpyAsync(out, p->outd, ne * Tt * 4, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (n_embeds) *n_embeds = (uint32_t)ne;
    return 0;
}
