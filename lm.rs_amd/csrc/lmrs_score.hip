// lmrs_score.hip — the reduction behind lmrs_score_tokens (include/lmrs_hip.h): over each row of a [tokens][vocab] block of logits, the
// first index of the f32 maximum (Sampler::sample_argmax, sampler.rs:29-41) and the log-softmax of a target token, in double.
//
// Two launches.  score_chunk_kernel: one workgroup of 256 lanes per 2048 logits of a row - two float4 loads per lane, the values stay in
// registers - forms the chunk's maximum and its first index, then sum exp((double)l - chunk max) over the chunk: one pass over HBM.
// score_merge_kernel: one wave per row merges the chunk summaries (maximum, first index, sum_c s_c * exp(max_c - max)) and forms
// l[y] - max - log(sum).  Llama's 128 256 logits are 63 workgroups per row: one token alone spreads over a quarter of the chip's CUs,
// 512 tokens over 32 k workgroups.  The rescaled sum differs from a direct sum of exp(l - max) by a few double ulps, far below the f32
// rounding of the result.  The summation order depends on the vocabulary size alone: a row gives the same bits in any launch.
//
// topk_chunk_kernel / topk_merge_kernel: the k first candidates of every row over the same chunking (lmrs_score_tokens_topk, lmrs_forward_topk):
// described where they stand.
//
// softcap_rows_kernel: Gemma-2's soft-cap of the first `dim` logits of every row of the block, between the batched classifier GEMM and the
// reduction (the decode classifier applies it in its epilogue).
//
// mask_rows_kernel: a batch slot's allowed-token mask (lmrs_batch_set_masks) over the rows of the block, behind the soft-cap and in front of every
// sink: -inf over the disallowed logits.  Stores only.
//
// automaton_masks_kernel / auto_rows_mask_kernel: a token automaton's per-state masks built from its tables (lmrs_batch_automaton_create), and
// mask_rows_kernel with the row's mask found through the slot's state word on the device; gen_advance_kernel moves that word at the step boundary.
//
// record_rows_kernel / penalty_rows_kernel: a batch's token record per slot and the repetition / presence / frequency penalties over it
// (lmrs_batch_set_penalties), between the soft-cap and the mask: one workgroup a penalised row sorts the row's record in LDS and changes one logit per
// distinct token.
//
// filter_rows_kernel: a batch slot's candidate filters (lmrs_batch_set_filters) - top_k by an exact radix select over the row's 64-bit keys, min_gap below the
// row's first candidate - behind the masks and in front of every sink: one workgroup a filtered row, -inf stores only.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "lmrs_score.h"

namespace lmrs {
namespace {

constexpr int kLanes = 256;
constexpr int kPerLane = kScoreChunk / kLanes;          // 8: two float4
static_assert(kPerLane == 8, "a lane holds two float4 of its chunk");

// (value, index) pairs: the larger value wins, equal values -> the lower index (the first maximum).  No NaN reaches these.
__device__ __forceinline__ void take_max(float& m, int& i, float om, int oi) {
    if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}
__device__ __forceinline__ void wave_max(float& m, int& i) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) take_max(m, i, __shfl_xor(m, off), __shfl_xor(i, off));
}
// butterfly: every lane ends with the same sum (a + b == b + a), the order fixed by the lane numbering
__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// A lane's eight logits of the chunk at c0: element e is column chunk_index(c0, tid, e); columns from `written` on read as 0.0 (past `vocab`: the
// caller masks them).  VEC: rows start 16-byte aligned (ld % 4 == 0): float4 loads wherever four written values are whole
__device__ __forceinline__ int chunk_index(int c0, int tid, int e) { return c0 + 4 * (tid + (e >> 2) * kLanes) + (e & 3); }
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float* row, int c0, int written, int tid, float (&v)[kPerLane]) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i0 = c0 + 4 * (tid + k * kLanes);
        if (VEC && i0 + 3 < written) {
            const float4 f = *reinterpret_cast<const float4*>(row + i0);
            v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[4 * k + j] = i0 + j < written ? row[i0 + j] : 0.0f;
        }
    }
}

// grid (chunks of the row, rows)
template <bool VEC>
__global__ __launch_bounds__(kLanes) void score_chunk_kernel(const ScoreArgs a) {
    __shared__ float s_max[kLanes / 64];
    __shared__ int s_idx[kLanes / 64];
    __shared__ double s_sum[kLanes / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* row = a.logits + (size_t)blockIdx.y * a.ld;
    const int c0 = blockIdx.x * kScoreChunk;
    float v[kPerLane];
    load_chunk<VEC>(row, c0, a.written, tid, v);
    // the lane's first maximum (its indices ascend), NaNs skipped; then the workgroup's
    float m = -INFINITY; int mi = INT_MAX;
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int i = chunk_index(c0, tid, e);
        if (i < a.vocab && v[e] == v[e] && (v[e] > m || mi == INT_MAX)) { m = v[e]; mi = i; }
    }
    wave_max(m, mi);
    if (lane == 0) { s_max[wave] = m; s_idx[wave] = mi; }
    __syncthreads();
    m = s_max[0]; mi = s_idx[0];
#pragma unroll
    for (int w = 1; w < kLanes / 64; ++w) take_max(m, mi, s_max[w], s_idx[w]);
    // sum of exp(l - chunk max) in double (a chunk of -inf / NaN only: 0)
    double s = 0.0;
    if (m != -INFINITY) {
        const double md = (double)m;
#pragma unroll
        for (int e = 0; e < kPerLane; ++e) {
            const int i = chunk_index(c0, tid, e);
            if (i < a.vocab) s += exp((double)v[e] - md);
        }
    }
    s = wave_sum(s);
    if (lane == 0) s_sum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        ScorePart p; p.max = m; p.idx = mi; p.sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
        a.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// One wave merges a row's S chunk summaries: the f32 maximum m, its first index mi (INT_MAX: no number in the row) and
// s = sum_c s_c * exp(max_c - m) in double; every lane ends with the same three
__device__ __forceinline__ void row_max_sum(const ScorePart* pp, int S, int lane, float& m, int& mi, double& s) {
    m = -INFINITY; mi = INT_MAX;
    for (int c = lane; c < S; c += 64) take_max(m, mi, pp[c].max, pp[c].idx);
    wave_max(m, mi);
    const double md = (double)m;
    s = 0.0;
    for (int c = lane; c < S; c += 64) {
        const ScorePart q = pp[c];
        if (q.max != -INFINITY) s += q.sum * exp((double)q.max - md);
    }
    s = wave_sum(s);
}

// the log-softmax of a row at a logit ly: md = the row's f32 maximum widened, s = row_max_sum's sum (score_merge_kernel and gen_logprobs_kernel: one copy)
__device__ __forceinline__ double log_softmax_at(float ly, double md, double s) { return (double)ly - md - log(s); }

// one wave per row (four rows per workgroup)
__global__ __launch_bounds__(kLanes) void score_merge_kernel(const ScoreArgs a) {
    const int r = blockIdx.x * (kLanes / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= a.rows) return;                                                // (wave-uniform)
    const int S = score_chunks(a.vocab);
    float m; int mi; double s;
    row_max_sum(a.part + (size_t)r * S, S, lane, m, mi, s);
    const double md = (double)m;
    if (lane == 0) {
        const float* row = a.logits + (size_t)r * a.ld;
        const float l0 = a.written > 0 ? row[0] : 0.0f;
        a.out_idx[r] = l0 != l0 || mi == INT_MAX ? 0u : (uint32_t)mi;     // a NaN at index 0 is never displaced (strict `>` from index 0)
        if (r < a.n_tgt) {
            const uint32_t y = a.tgt[r];
            const float ly = y < (uint32_t)a.written ? row[y] : 0.0f;
            a.out_lp[r] = log_softmax_at(ly, md, s);
        }
    }
}

// ------------------------------------------------------------------ top-k of every row (launch_topk_rows)
// Every entry becomes one 64-bit key whose descending order IS the candidate order of lmrs_score.h: the value's bits made monotone in the high word
// (-0.0 folded onto +0.0, a NaN 0 - below -inf -, a NaN at index 0 the largest word of all), ~index in the low word.  Keys are unique and never 0.
// Two launches over the scores' chunking.  topk_chunk_kernel: a workgroup finds the min(k, entries)-th largest key of its 2048 by a radix select,
// eight bits a round from the top (a 256-bin count in LDS, one bin per lane; it stops at the first round whose bin is wanted whole: two or three
// rounds on ordinary logits), and writes the keys from there up to its k slots (0 fills a short chunk): one pass over HBM.  topk_merge_kernel: a
// workgroup per row runs the same select for the k-th key of the row's S * k candidates and places each survivor at the number of survivors above
// it.  The slot a key lands in between the two depends on the order of arrival; the select and the placement look at key values alone, so
// nothing that is written out does.  The counts are integer sums.
__device__ __forceinline__ unsigned long long topk_key(float f, int i) {
    unsigned b = __float_as_uint(f), hi;
    if (f != f) hi = i == 0 ? 0xFFFFFFFFu : 0u;
    else {
        if (b == 0x80000000u) b = 0u;
        hi = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    }
    return ((unsigned long long)hi << 32) | (unsigned)~(unsigned)i;
}

struct SelectLds { unsigned hist[kLanes]; unsigned wtot[kLanes / 64]; unsigned pick[3]; };

// The workgroup's r-th largest of keys[0 .. n) (all lanes call it; 1 <= r <= the number of non-zero keys, which are unique), or that key with its
// low bits cleared when every key sharing the bits above is wanted: `key >= the result` holds for exactly r keys.
__device__ __forceinline__ unsigned long long block_kth_key(const unsigned long long* keys, int n, unsigned r, SelectLds& L) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long pfx = 0, known = 0;                                  // the bits decided so far, and their mask
    for (int shift = 56; shift >= 0; shift -= 8) {
        L.hist[tid] = 0;
        __syncthreads();
        for (int j = tid; j < n; j += kLanes) {
            const unsigned long long key = keys[j];
            if ((key & known) == pfx) atomicAdd(&L.hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        // lane = bin: the keys in higher bins, by a suffix sum over the wave and the waves' totals
        const unsigned h = L.hist[tid];
        unsigned x = h;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned y = __shfl_down(x, off); if (lane + off < 64) x += y; }
        if (lane == 0) L.wtot[wave] = x;
        __syncthreads();
        unsigned above = x - h;
        for (int w = wave + 1; w < kLanes / 64; ++w) above += L.wtot[w];
        if (above < r && r <= above + h) { L.pick[0] = (unsigned)tid; L.pick[1] = r - above; L.pick[2] = h; }   // (one bin)
        __syncthreads();
        pfx |= (unsigned long long)L.pick[0] << shift; known |= 0xFFull << shift;
        r = L.pick[1];
        if (r == L.pick[2]) break;                                          // the whole bin is wanted (at shift 0: the one key)
    }
    return pfx;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned s) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

static_assert(kTopkMax <= kLanes, "a lane per candidate slot");

// grid (chunks of the row, rows), as score_chunk_kernel
template <bool VEC>
__global__ __launch_bounds__(kLanes) void topk_chunk_kernel(const TopkArgs a) {
    __shared__ unsigned long long s_keys[kScoreChunk];
    __shared__ SelectLds s_sel;
    __shared__ unsigned s_n[2];                                             // slots handed out; keys ahead of the target
    const int tid = threadIdx.x;
    const float* row = a.logits + (size_t)blockIdx.y * a.ld;
    const int c0 = blockIdx.x * kScoreChunk;
    float v[kPerLane];
    load_chunk<VEC>(row, c0, a.written, tid, v);
    if (tid < 2) s_n[tid] = 0;
    unsigned long long key[kPerLane];
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
        const int i = chunk_index(c0, tid, e);
        key[e] = i < a.vocab ? topk_key(v[e], i) : 0ull;
        s_keys[e * kLanes + tid] = key[e];
    }
    const bool ranked = a.out_rank && (int)blockIdx.y < a.n_tgt;            // (uniform)
    unsigned ahead = 0;
    if (ranked) {
        const uint32_t y = a.tgt[blockIdx.y];
        const unsigned long long ky = topk_key(y < (uint32_t)a.written ? row[y] : 0.0f, (int)y);
#pragma unroll
        for (int e = 0; e < kPerLane; ++e) ahead += key[e] > ky;
        ahead = wave_sum_u32(ahead);
    }
    __syncthreads();
    if (ranked && (tid & 63) == 0) atomicAdd(&s_n[1], ahead);
    const unsigned r = (unsigned)min(a.k, min(kScoreChunk, a.vocab - c0));
    const unsigned long long kth = block_kth_key(s_keys, kScoreChunk, r, s_sel);
    const size_t part = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    unsigned long long* out = a.cand + part * a.k;
#pragma unroll
    for (int e = 0; e < kPerLane; ++e)
        if (key[e] >= kth) {
            const unsigned slot = atomicAdd(&s_n[0], 1u);
            if (slot < r) out[slot] = key[e];
        }
    if (tid >= (int)r && tid < a.k) out[tid] = 0ull;
    if (ranked && tid == 0) a.cnt[part] = s_n[1];                           // (complete: the select's barriers lie behind the four adds)
}

// one workgroup per row
__global__ __launch_bounds__(kLanes) void topk_merge_kernel(const TopkArgs a) {
    __shared__ unsigned long long s_top[kTopkMax];
    __shared__ SelectLds s_sel;
    __shared__ unsigned s_n;
    const int tid = threadIdx.x, lane = tid & 63, r = blockIdx.x, S = score_chunks(a.vocab), n = S * a.k;
    const unsigned long long* cand = a.cand + (size_t)r * n;
    if (tid == 0) s_n = 0;
    const unsigned long long kth = block_kth_key(cand, n, (unsigned)a.k, s_sel);
    for (int j = tid; j < n; j += kLanes) {
        const unsigned long long key = cand[j];
        if (key >= kth) {
            const unsigned slot = atomicAdd(&s_n, 1u);
            if (slot < (unsigned)a.k) s_top[slot] = key;
        }
    }
    __syncthreads();
    double md = 0.0, ls = 0.0;
    if (a.part) {                                                           // the row's m and log(sum) as score_merge_kernel forms them
        float m; int mi; double s;
        row_max_sum(a.part + (size_t)r * S, S, lane, m, mi, s);
        md = (double)m; ls = log(s);
    }
    if (tid < a.k) {
        const unsigned long long key = s_top[tid];
        int rank = 0;
        for (int i = 0; i < a.k; ++i) rank += s_top[i] > key;
        const uint32_t idx = ~(uint32_t)key;
        const float l = idx < (uint32_t)a.written ? a.logits[(size_t)r * a.ld + idx] : 0.0f;
        a.out_idx[(size_t)r * a.k + rank] = idx;
        a.out_val[(size_t)r * a.k + rank] = a.part ? (float)((double)l - md - ls) : l;
    }
    if (a.out_rank && r < a.n_tgt && tid < 64) {
        unsigned ahead = 0;
        for (int c = lane; c < S; c += 64) ahead += a.cnt[(size_t)r * S + c];
        ahead = wave_sum_u32(ahead);
        if (lane == 0) a.out_rank[r] = ahead;
    }
}

// Gemma-2's soft-cap of the first `cols` logits (transformer.rs:375-381) over a block of rows: l / 30, (float)tanh((double)l), * 30 - the three
// roundings of the decode classifier's epilogue (EPI_CLS, lmrs_kernels.hip) with the same device tanh, so a row carries the decode step's bits.
// grid (ceil(cols / 256), rows)
__global__ __launch_bounds__(kLanes) void softcap_rows_kernel(float* logits, int ld, int cols) {
    const int i = blockIdx.x * kLanes + threadIdx.x;
    if (i >= cols) return;
    float* p = logits + (size_t)blockIdx.y * ld + i;
    float v = *p;
    v = v / 30.0f;
    v = (float)tanh((double)v);
    v = v * 30.0f;
    *p = v;
}

// Row blockIdx.y of the block under mask row mask_of[blockIdx.y] of `bits` (`words` words a mask; < 0: the row has no mask and its workgroup leaves).
// No logit is read.  A lane owns four consecutive columns - one aligned 16-byte store - and the four bits of them in the mask word it shares with
// seven neighbours: all set, nothing; none set, one float4 of -inf; mixed, a dword store per cleared bit.  A wave covers 256 columns: eight mask
// words, 1 KB of contiguous stores.  cols % 4 == 0, so no lane's four straddle the row's end.
__global__ __launch_bounds__(kLanes) void mask_rows_kernel(float* logits, int ld, int cols, const uint32_t* bits, int words, const int* mask_of) {
    const int m = mask_of[blockIdx.y];
    if (m < 0) return;
    const int g = blockIdx.x * kLanes + threadIdx.x;
    if (4 * g >= cols) return;
    const uint32_t allowed = bits[(size_t)m * words + (g >> 3)] >> ((g & 7) * 4) & 15u;
    if (allowed == 15u) return;
    float* p = logits + (size_t)blockIdx.y * ld + 4 * g;
    const float ninf = -INFINITY;
    if (allowed == 0u) { *reinterpret_cast<float4*>(p) = make_float4(ninf, ninf, ninf, ninf); return; }
    if (!(allowed & 1u)) p[0] = ninf;
    if (!(allowed & 2u)) p[1] = ninf;
    if (!(allowed & 4u)) p[2] = ninf;
    if (!(allowed & 8u)) p[3] = ninf;
}

// mask_rows_kernel with the mask found on the device (a slot with a token automaton): the row's mask is the one of the state its slot stands in NOW,
// masks + state[slot] * words - one more dependent load per workgroup, then the same bits, the same four columns a lane and the same stores.  Inside the
// device loop the state word is what gen_advance_kernel left behind the pass before: the host names the slot once and never the state.
__global__ __launch_bounds__(kLanes) void auto_rows_mask_kernel(float* logits, int ld, int cols, const AutoRow* of, const uint32_t* state, int words) {
    const AutoRow a = of[blockIdx.y];
    if (a.slot < 0) return;
    const uint32_t q = state[a.slot];
    if (q >= a.n_states) return;
    const int g = blockIdx.x * kLanes + threadIdx.x;
    if (4 * g >= cols) return;
    const uint32_t allowed = a.masks[(size_t)q * words + (g >> 3)] >> ((g & 7) * 4) & 15u;
    if (allowed == 15u) return;
    float* p = logits + (size_t)blockIdx.y * ld + 4 * g;
    const float ninf = -INFINITY;
    if (allowed == 0u) { *reinterpret_cast<float4*>(p) = make_float4(ninf, ninf, ninf, ninf); return; }
    if (!(allowed & 1u)) p[0] = ninf;
    if (!(allowed & 2u)) p[1] = ninf;
    if (!(allowed & 4u)) p[2] = ninf;
    if (!(allowed & 8u)) p[3] = ninf;
}

// The masks of an automaton's states from its tables (lmrs_batch_automaton_create): one token per lane, a wave's 64 tokens two mask words by a ballot.
// A lane reads its token's class ONCE and keeps it; the workgroup then walks the states of its grid row (q = blockIdx.y, + gridDim.y, ...), one load from the
// state's `next` row per lane and state - rows of a few classes sit in one or two cache lines.  Lane 0 of a wave stores the wave's two words; a token at or
// above `vocab` votes 0, so the bits at and above vocab_size are clear, and a word at or above `words` is not written.  grid (ceil(vocab / 256), states)
__global__ __launch_bounds__(kLanes) void automaton_masks_kernel(const uint16_t* class_of, const uint32_t* next, int vocab, uint32_t n_states, uint32_t n_classes,
                                                                 uint32_t* bits, int words) {
    const int t = blockIdx.x * kLanes + threadIdx.x;
    const int w0 = (t >> 6) * 2;                                            // the wave's first word (wave-uniform: kLanes % 64 == 0)
    if (w0 >= words) return;
    const bool in = t < vocab;
    const uint32_t c = in ? class_of[t] : 0u;
    for (uint32_t q = blockIdx.y; q < n_states; q += gridDim.y) {
        const bool live = in && next[(size_t)q * n_classes + c] != kAutoDead;
        const unsigned long long m = __ballot(live);
        if ((threadIdx.x & 63) == 0) {
            uint32_t* p = bits + (size_t)q * words + w0;
            p[0] = (uint32_t)m;
            if (w0 + 1 < words) p[1] = (uint32_t)(m >> 32);
        }
    }
}

// The token record of a batch (lmrs_batch_set_history): table row r wrote K/V at position pos[r] of slot slot_of[r], so hist[slot][pos] = its token -
// kTokenNone for an embedding row (a source word with the stage bit, lmrs_kernels.h).  One lane a row; two rows of one launch never share a (slot, position).
__global__ __launch_bounds__(kLanes) void record_rows_kernel(uint32_t* hist, int seq_len, int n_slots, const int* pos, const uint32_t* tok, const int* slot_of, int n_rows) {
    const int r = blockIdx.x * kLanes + threadIdx.x;
    if (r >= n_rows) return;
    const int s = slot_of[r], p = pos[r];
    if (s < 0 || s >= n_slots || p < 0 || p >= seq_len) return;
    const uint32_t w = tok[r];
    hist[(size_t)s * seq_len + p] = (w & 0x80000000u) ? kTokenNone : w;
}

// Row blockIdx.x of the block under the penalties of its slot (lmrs_batch_set_penalties; rows[blockIdx.x].slot < 0: none, the workgroup leaves).  p = the
// position of the row as the device table has it NOW (pos[rows[..].tab_row]: inside lmrs_batch_generate_greedy's loop the host does not know it).
// 1. the record hist[slot][0 .. p] into LDS as keys (token << 1) | (i >= out_from), kTokenNone as the all-ones key, padded with it to a power of two;
// 2. a bitonic network over the keys, ascending: the occurrences of a token become one run, those in front of out_from first;
// 3. the lane that holds the head of a run finds the run's end and the first key of it with the low bit by binary search - c_all and c_out are differences of
//    indices, integers whatever the order the lanes arrive in - and is the ONE thread that reads, changes and writes that logit: an IEEE division or a
//    product, then a product, a difference and a difference, each rounded once (the object is built with -ffp-contract=off).
// cap: the power of two the launch's LDS holds, >= every row's p + 1.
__global__ __launch_bounds__(kLanes) void penalty_rows_kernel(float* logits, int ld, int cols, const uint32_t* hist, int seq_len, const int* pos, const PenaltyRow* rows, int cap) {
    extern __shared__ uint32_t keys[];
    const PenaltyRow pr = rows[blockIdx.x];
    if (pr.slot < 0) return;
    const int p = pos[pr.tab_row];
    if (p < 0 || p >= seq_len || p >= cap) return;
    int N = 2;
    while (N < p + 1) N <<= 1;
    const uint32_t* h = hist + (size_t)pr.slot * seq_len;
    const int tid = threadIdx.x;
    for (int i = tid; i < N; i += kLanes) {
        const uint32_t t = i <= p ? h[i] : kTokenNone;
        keys[i] = t == kTokenNone ? kTokenNone : (t << 1 | ((uint32_t)i >= pr.out_from ? 1u : 0u));
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < N / 2; t += kLanes) {
                const int lo = 2 * t - (t & (j - 1)), hi = lo + j;                  // the t-th pair of the stage: lo has bit j clear
                const uint32_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    float* row = logits + (size_t)blockIdx.x * ld;
    for (int i = tid; i < N; i += kLanes) {
        const uint32_t key = keys[i];
        if (key == kTokenNone) continue;
        const uint32_t t = key >> 1;
        if ((i > 0 && keys[i - 1] >> 1 == t) || t >= (uint32_t)cols) continue;
        // first index in (i, N] whose key is >= bound (the padding is above every token's keys)
        auto first_at_least = [&](uint32_t bound) {
            int a = i, b = N;
            while (a < b) { const int mid = (a + b) >> 1; if (keys[mid] < bound) a = mid + 1; else b = mid; }
            return a;
        };
        const int end = first_at_least((t + 1) << 1), out0 = first_at_least(t << 1 | 1u);
        const int c_out = end - out0;                                               // (c_all = end - i >= 1: the head itself)
        float l = row[t];
        if (pr.repetition != 1.0f) l = l > 0.0f ? __fdiv_rn(l, pr.repetition) : __fmul_rn(l, pr.repetition);
        if (c_out > 0) l = __fsub_rn(__fsub_rn(l, __fmul_rn(pr.frequency, (float)c_out)), pr.presence);
        row[t] = l;
    }
}

// ------------------------------------------------------------------ a slot's candidate filters over its rows (launch_filter_rows)
// One workgroup of 1024 lanes a filtered row (sixteen waves keep a CU's loads in flight; a row of 128 256 logits is 32 trips of float4 a lane), the row read
// from L2 behind its first pass.  top_k: block_kth_key's radix select, eight bits a round from the top of topk_key's 64-bit keys, but over the row itself -
// the keys are formed again from the logits at every round, so there is no vocabulary-sized scratch and no limit on k; the rounds stop at the first bin that
// is wanted whole (three or four rounds on ordinary logits: the value's 32 bits, rarely a tie at the threshold), and a round over index bits that are the
// same in every key of the row (~i above the row's width) is not run.  Rows of equal values take every round - the worst case - so a wave first adds the
// bins most of its lanes share by one atomic each (two peels), then the rest lane by lane: LDS atomics on one address serialise.  min_gap: the largest value
// word, taken along in the first round (a pass of its own for a row without top_k), then m - min_gap.  Then one pass of stores, -inf only.
constexpr int kFilterLanes = 1024;
struct FilterLds { unsigned hist[256]; unsigned wtot[4]; unsigned pick[3]; unsigned red[kFilterLanes / 64]; };

// every entry of the row once, in trips that all lanes of the workgroup make together (the ballots of wave_bin_add see whole waves): f(value, index, valid).
// vec: the row starts 16-byte aligned - float4 loads over its whole fours
template <class F>
__device__ __forceinline__ void filter_each(const float* row, int n, bool vec, F&& f) {
    const int tid = threadIdx.x;
    int done = 0;
    if (vec) {
        const int n4 = n >> 2;
        for (int base = 0; base < n4; base += kFilterLanes) {
            const int j = base + tid;
            const bool ok = j < n4;
            const float4 v = ok ? reinterpret_cast<const float4*>(row)[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            f(v.x, 4 * j, ok); f(v.y, 4 * j + 1, ok); f(v.z, 4 * j + 2, ok); f(v.w, 4 * j + 3, ok);
        }
        done = n4 * 4;
    }
    for (int base = done; base < n; base += kFilterLanes) {
        const int i = base + tid;
        const bool ok = i < n;
        f(ok ? row[i] : 0.0f, i, ok);
    }
}

// hist[bin] += 1 for every lane of the wave that wants it (bin < 256 in every lane): the first wanting lane's bin by one atomic for all lanes that share it,
// twice, then an atomic a lane - integer sums, the same totals in any order
__device__ __forceinline__ void wave_bin_add(unsigned* hist, unsigned bin, bool want) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(want);
    for (int it = 0; it < 2 && todo; ++it) {
        const int lead = __ffsll((unsigned long long)todo) - 1;
        const unsigned lb = __shfl(bin, lead);
        const unsigned long long same = __ballot(want && bin == lb);
        if (lane == lead) atomicAdd(&hist[lb], (unsigned)__popcll(same));
        if (bin == lb) want = false;
        todo &= ~same;
    }
    if (want) atomicAdd(&hist[bin], 1u);
}

__global__ __launch_bounds__(kFilterLanes) void filter_rows_kernel(float* logits, int ld, int cols, const FilterRow* rows) {
    __shared__ FilterLds L;
    const FilterRow fr = rows[blockIdx.x];
    if (fr.slot < 0) return;
    const bool tk = fr.top_k != 0u && fr.top_k < (unsigned)cols;
    const bool gap = fr.min_gap < INFINITY;                                 // (a NaN: off)
    if (!tk && !gap) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* row = logits + (size_t)blockIdx.x * ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    unsigned mx = 0;                                                        // the largest value word the lane has seen (never 0 over a whole row)
    unsigned long long kth = 0;                                             // key >= kth: among the first top_k candidates
    if (tk) {
        unsigned long long pfx = 0, known = 0;
        unsigned r = fr.top_k;                                              // 1 <= r <= the keys that share the bits decided so far, throughout
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (shift < 32 && ((unsigned)(cols - 1) >> shift) == 0u) {      // ~i has this byte all ones in every key of the row
                pfx |= 0xFFull << shift; known |= 0xFFull << shift;
                continue;
            }
            if (tid < 256) L.hist[tid] = 0;
            __syncthreads();
            filter_each(row, cols, vec, [&](float v, int i, bool ok) {
                const unsigned long long key = topk_key(v, i);
                if (shift == 56 && ok) mx = max(mx, (unsigned)(key >> 32));
                wave_bin_add(L.hist, (unsigned)(key >> shift) & 255u, ok && (key & known) == pfx);
            });
            __syncthreads();
            // lane = bin (the first four waves): the keys in higher bins, by a suffix sum over the wave and the waves' totals - block_kth_key's
            unsigned h = 0, x = 0;
            if (tid < 256) {
                h = L.hist[tid]; x = h;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const unsigned y = __shfl_down(x, off); if (lane + off < 64) x += y; }
                if (lane == 0) L.wtot[wave] = x;
            }
            __syncthreads();
            if (tid < 256) {
                unsigned above = x - h;
                for (int w = wave + 1; w < 4; ++w) above += L.wtot[w];
                if (above < r && r <= above + h) { L.pick[0] = (unsigned)tid; L.pick[1] = r - above; L.pick[2] = h; }   // (one bin)
            }
            __syncthreads();
            pfx |= (unsigned long long)L.pick[0] << shift; known |= 0xFFull << shift;
            r = L.pick[1];
            if (r == L.pick[2]) break;                                      // the whole bin is wanted (at shift 0: the one key)
        }
        kth = pfx;
    }
    bool use_gap = false;
    float thr = 0.0f;
    if (gap) {
        if (!tk) filter_each(row, cols, vec, [&](float v, int i, bool ok) { if (ok) mx = max(mx, (unsigned)(topk_key(v, i) >> 32)); });
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = max(mx, (unsigned)__shfl_xor(mx, off));
        if (lane == 0) L.red[wave] = mx;
        __syncthreads();
        mx = L.red[0];
#pragma unroll
        for (int w = 1; w < kFilterLanes / 64; ++w) mx = max(mx, L.red[w]);
        // the first candidate's value from its word; all ones: a NaN at index 0 - nothing is cleared by the gap
        use_gap = mx != 0xFFFFFFFFu && mx != 0u;
        const unsigned mb = (mx & 0x80000000u) ? (mx & 0x7FFFFFFFu) : ~mx;
        thr = __fsub_rn(__uint_as_float(mb), fr.min_gap);
    }
    auto cut = [&](float v, int i) { return (tk && topk_key(v, i) < kth) || (use_gap && !(v >= thr)); };
    const unsigned kNinfBits = 0xFF800000u;
    const float ninf = -INFINITY;
    int done = 0;
    if (vec) {
        const int n4 = cols >> 2;
        for (int j = tid; j < n4; j += kFilterLanes) {
            float* p = row + 4 * j;
            const float4 v = *reinterpret_cast<const float4*>(p);
            const bool c0 = cut(v.x, 4 * j), c1 = cut(v.y, 4 * j + 1), c2 = cut(v.z, 4 * j + 2), c3 = cut(v.w, 4 * j + 3);
            const bool w0 = c0 && __float_as_uint(v.x) != kNinfBits, w1 = c1 && __float_as_uint(v.y) != kNinfBits,
                       w2 = c2 && __float_as_uint(v.z) != kNinfBits, w3 = c3 && __float_as_uint(v.w) != kNinfBits;
            if (c0 && c1 && c2 && c3) {
                if (w0 || w1 || w2 || w3) *reinterpret_cast<float4*>(p) = make_float4(ninf, ninf, ninf, ninf);
                continue;
            }
            if (w0) p[0] = ninf;
            if (w1) p[1] = ninf;
            if (w2) p[2] = ninf;
            if (w3) p[3] = ninf;
        }
        done = n4 * 4;
    }
    for (int i = done + tid; i < cols; i += kFilterLanes) {
        const float v = row[i];
        if (cut(v, i) && __float_as_uint(v) != kNinfBits) row[i] = ninf;
    }
}

// ------------------------------------------------------------------ the step boundary of lmrs_batch_generate's device loop (launch_gen_advance / launch_gen_logprobs)
__device__ __forceinline__ uint32_t gen_picked(const GenRow& g, const GenPick& pick, int o) {
    return g.from_samp ? (uint32_t)pick.samp[(size_t)o * pick.samp_ld] : pick.idx[o];
}
// one lane per output row; sel null: the row table (output o is table row o), else the long table's sel column
// AUTO: some row of the pass has a token automaton (aut[o].slot >= 0: output o's; state: the batch's state words).  Such a live row takes two dependent loads
// more - class_of[t], then next[q][class] - and nobody else does; without AUTO the kernel is, instruction for instruction, the one it was before automata.
// q' dead (the row chose a token its mask had cleared: a row without a number among the allowed) moves nothing: the host's walk reports it.
// (one body, two kernels under names of their own: gen_advance_kernel is the AUTO = false instance and takes the arguments it always took)
template <bool AUTO>
__device__ __forceinline__ void gen_advance_rows(GenRow* st, int* pos, uint32_t* tok, const uint32_t* sel, const GenPick& pick, uint32_t* out,
                                                 uint32_t* n_live, int n_rows, const AutoRow* aut, uint32_t* state) {
    const int o = threadIdx.x;
    bool live = false;
    if (o < n_rows) {
        // everything the lane may need is asked for at once, whether or not the row is live: the launch is one round trip to memory deep (two through sel),
        // as table_advance_kernel / runs_advance_kernel are
        const GenRow g = st[o];
        const uint32_t ti = pick.idx[o], ts = pick.samp ? (uint32_t)pick.samp[(size_t)o * pick.samp_ld] : 0u;
        const uint32_t r = sel ? sel[o] : (uint32_t)o;
        const int p = pos[r];
        AutoRow a{}; a.slot = -1;
        if (AUTO) a = aut[o];
        if (g.live) {
            const uint32_t t = g.from_samp ? ts : ti, done = g.done + 1;
            out[g.out_at + g.done] = t;
            bool stop = false;
#pragma unroll
            for (int k = 0; k < kGenStopMax; ++k) stop = stop || ((uint32_t)k < g.n_stop && g.stop[k] == t);
            uint32_t nx = kAutoDead;
            if (AUTO && a.slot >= 0) {
                const uint32_t q = state[a.slot];
                if (q < a.n_states && t < a.vocab) {
                    const uint32_t c = a.class_of[t];
                    if (c < a.n_classes) nx = a.next[(size_t)q * a.n_classes + c];
                }
            }
            st[o].done = done; st[o].last = t;
            if (stop) { st[o].live = 0; st[o].finish = 1; }
            else if (AUTO && nx != kAutoDead && (nx & kAutoFinalBit)) { st[o].live = 0; st[o].finish = kGenFinishFinal; }
            else if (done >= g.budget) { st[o].live = 0; st[o].finish = 0; }
            else {
                tok[r] = t; pos[r] = p + 1; live = true;
                if (AUTO && nx != kAutoDead) state[a.slot] = nx & ~kAutoFinalBit;
            }
        }
    }
    const unsigned long long m = __ballot(live);
    if (o == 0) *n_live = (uint32_t)__popcll(m);
}
__global__ __launch_bounds__(kGenRowsMax) void gen_advance_kernel(GenRow* st, int* pos, uint32_t* tok, const uint32_t* sel, const GenPick pick, uint32_t* out,
                                                                  uint32_t* n_live, int n_rows) {
    gen_advance_rows<false>(st, pos, tok, sel, pick, out, n_live, n_rows, nullptr, nullptr);
}
__global__ __launch_bounds__(kGenRowsMax) void gen_advance_auto_kernel(GenRow* st, int* pos, uint32_t* tok, const uint32_t* sel, const GenPick pick, uint32_t* out,
                                                                       uint32_t* n_live, int n_rows, const AutoRow* aut, uint32_t* state) {
    gen_advance_rows<true>(st, pos, tok, sel, pick, out, n_live, n_rows, aut, state);
}
// one wave per output row (four rows per workgroup)
__global__ __launch_bounds__(kLanes) void gen_logprobs_kernel(const GenRow* st, const GenPick pick, const float* logits, int ld, int vocab, const ScorePart* part,
                                                             float* lp_out, int n_rows) {
    const int o = blockIdx.x * (kLanes / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= n_rows || !st[o].live) return;                                 // (wave-uniform)
    const int S = score_chunks(vocab);
    float m; int mi; double s;
    row_max_sum(part + (size_t)o * S, S, lane, m, mi, s);
    if (lane == 0) {
        const GenRow g = st[o];
        const uint32_t t = gen_picked(g, pick, o);
        const float ly = t < (uint32_t)vocab ? logits[(size_t)o * ld + t] : 0.0f;
        lp_out[g.out_at + g.done] = (float)log_softmax_at(ly, (double)m, s);
    }
}

}  // namespace

hipError_t launch_gen_advance(GenRow* st, int* pos, uint32_t* tok, const uint32_t* sel, GenPick pick, uint32_t* out, uint32_t* n_live, int n_rows, hipStream_t s,
                              const AutoRow* aut, uint32_t* state) {
    if (!st || !pos || !tok || !pick.idx || !out || !n_live || n_rows < 1 || n_rows > kGenRowsMax || (aut && !state)) return hipErrorInvalidValue;
    if (aut) hipLaunchKernelGGL(gen_advance_auto_kernel, dim3(1), dim3(kGenRowsMax), 0, s, st, pos, tok, sel, pick, out, n_live, n_rows, aut, state);
    else hipLaunchKernelGGL(gen_advance_kernel, dim3(1), dim3(kGenRowsMax), 0, s, st, pos, tok, sel, pick, out, n_live, n_rows);
    return hipGetLastError();
}
hipError_t launch_automaton_masks(const uint16_t* class_of, const uint32_t* next, int vocab, uint32_t n_states, uint32_t n_classes, uint32_t* bits, hipStream_t s) {
    if (!class_of || !next || !bits || vocab <= 0 || n_states < 1 || n_states >= kAutoFinalBit || n_classes < 1 || n_classes > 65536u) return hipErrorInvalidValue;
    const int words = (vocab + 31) / 32;
    hipLaunchKernelGGL(automaton_masks_kernel, dim3((vocab + kLanes - 1) / kLanes, n_states < 4096u ? n_states : 4096u), dim3(kLanes), 0, s, class_of, next, vocab,
                       n_states, n_classes, bits, words);
    return hipGetLastError();
}
hipError_t launch_auto_mask_rows(float* logits, int ld, int cols, int rows, const AutoRow* of, const uint32_t* state, int words, hipStream_t s) {
    if (!logits || !of || !state || rows <= 0 || rows > 65535 || cols <= 0 || cols > ld || cols % 4 || ld % 4 || (size_t)words * 32 < (size_t)cols ||
        (reinterpret_cast<uintptr_t>(logits) & 15) != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(auto_rows_mask_kernel, dim3((cols / 4 + kLanes - 1) / kLanes, rows), dim3(kLanes), 0, s, logits, ld, cols, of, state, words);
    return hipGetLastError();
}
hipError_t launch_gen_logprobs(const GenRow* st, GenPick pick, const float* logits, int ld, int vocab, const ScorePart* part, float* lp_out, int n_rows, hipStream_t s) {
    if (!st || !pick.idx || !logits || !part || !lp_out || n_rows < 1 || n_rows > kGenRowsMax || vocab <= 0 || ld < vocab) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gen_logprobs_kernel, dim3((n_rows + kLanes / 64 - 1) / (kLanes / 64)), dim3(kLanes), 0, s, st, pick, logits, ld, vocab, part, lp_out, n_rows);
    return hipGetLastError();
}

hipError_t launch_record_rows(uint32_t* hist, int seq_len, int n_slots, const int* pos, const uint32_t* tok, const int* slot_of, int n_rows, hipStream_t s) {
    if (!hist || !pos || !tok || !slot_of || seq_len <= 0 || n_slots <= 0 || n_rows <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(record_rows_kernel, dim3((n_rows + kLanes - 1) / kLanes), dim3(kLanes), 0, s, hist, seq_len, n_slots, pos, tok, slot_of, n_rows);
    return hipGetLastError();
}

hipError_t launch_penalty_rows(float* logits, int ld, int cols, int rows, const uint32_t* hist, int seq_len, const int* pos, const PenaltyRow* of, int max_n, hipStream_t s) {
    if (!logits || !hist || !pos || !of || rows <= 0 || rows > 65535 || cols <= 0 || cols > ld || seq_len <= 0 || max_n <= 0 || max_n > seq_len || max_n > kPenaltyKeysMax)
        return hipErrorInvalidValue;
    int cap = 2;
    while (cap < max_n) cap <<= 1;
    hipLaunchKernelGGL(penalty_rows_kernel, dim3(rows), dim3(kLanes), (size_t)cap * 4, s, logits, ld, cols, hist, seq_len, pos, of, cap);
    return hipGetLastError();
}

hipError_t launch_filter_rows(float* logits, int ld, int cols, int rows, const FilterRow* of, hipStream_t s) {
    if (!logits || !of || rows <= 0 || rows > 65535 || cols <= 0 || cols > ld || cols > (1 << 30) || (reinterpret_cast<uintptr_t>(logits) & 3) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_rows_kernel, dim3(rows), dim3(kFilterLanes), 0, s, logits, ld, cols, of);
    return hipGetLastError();
}

hipError_t launch_softcap_rows(float* logits, int ld, int cols, int rows, hipStream_t s) {
    if (!logits || rows <= 0 || rows > 65535 || cols <= 0 || cols > ld) return hipErrorInvalidValue;
    hipLaunchKernelGGL(softcap_rows_kernel, dim3((cols + kLanes - 1) / kLanes, rows), dim3(kLanes), 0, s, logits, ld, cols);
    return hipGetLastError();
}

hipError_t launch_mask_rows(float* logits, int ld, int cols, int rows, const uint32_t* bits, int words, const int* mask_of, hipStream_t s) {
    if (!logits || !bits || !mask_of || rows <= 0 || rows > 65535 || cols <= 0 || cols > ld || cols % 4 || ld % 4 || (size_t)words * 32 < (size_t)cols ||
        (reinterpret_cast<uintptr_t>(logits) & 15) != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_rows_kernel, dim3((cols / 4 + kLanes - 1) / kLanes, rows), dim3(kLanes), 0, s, logits, ld, cols, bits, words, mask_of);
    return hipGetLastError();
}

hipError_t launch_score_rows(const ScoreArgs& a, hipStream_t s) {
    if (a.rows <= 0 || a.rows > 65535 || a.vocab <= 0 || a.written < 0 || a.written > a.vocab || a.ld < a.written || !a.part || !a.out_idx ||
        (a.n_tgt > 0 && (!a.tgt || !a.out_lp)))
        return hipErrorInvalidValue;
    const dim3 grid(score_chunks(a.vocab), a.rows);
    if (a.ld % 4 == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15) == 0) hipLaunchKernelGGL(score_chunk_kernel<true>, grid, dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(score_chunk_kernel<false>, grid, dim3(kLanes), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_merge_kernel, dim3((a.rows + kLanes / 64 - 1) / (kLanes / 64)), dim3(kLanes), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_topk_rows(const TopkArgs& a, hipStream_t s) {
    if (a.rows <= 0 || a.rows > 65535 || a.vocab <= 0 || a.written < 0 || a.written > a.vocab || a.ld < a.written || a.k < 1 || a.k > kTopkMax ||
        a.k > a.vocab || !a.logits || !a.cand || !a.out_idx || !a.out_val || (a.out_rank && a.n_tgt > 0 && (!a.tgt || !a.cnt)))
        return hipErrorInvalidValue;
    const dim3 grid(score_chunks(a.vocab), a.rows);
    if (a.ld % 4 == 0 && (reinterpret_cast<uintptr_t>(a.logits) & 15) == 0) hipLaunchKernelGGL(topk_chunk_kernel<true>, grid, dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(topk_chunk_kernel<false>, grid, dim3(kLanes), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(a.rows), dim3(kLanes), 0, s, a);
    return hipGetLastError();
}

}  // namespace lmrs
