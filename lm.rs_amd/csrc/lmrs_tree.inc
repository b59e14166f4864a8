// ------------------------------------------------------------------------------------------------
// The table pass over TOKEN TREES (lmrs_batch_forward_tree / lmrs_batch_accept_path; included by lmrs_kernels.hip behind lmrs_kv4.inc).  A row of the pass
// is one node of a tree of drafted tokens that hangs off position `base` of its slot.  The node has TWO positions: the LOGICAL one, base + depth, which
// rotates q and k and which Gemma's window and the length of the row's context see, and the STORAGE one, base + node index, where its K and V rows are
// kept - siblings share a logical position and may not share a cache row.  The row's context is the slot's positions 0 .. base - 1 as they stand, then its
// ancestors root-most first, then itself: T = base + depth + 1 keys, enumerated in logical order; key t < base lives at storage t, key t >= base at
// storage base + anc[t - base] (TreeRow::anc, one byte a key, self last).  The keys are COMPACTED, not masked: per (head, row) the scores, the max, the
// exps, the sequential sum, the divide, the products and the per-dim sequential value sum are paged_attention_body's over exactly these T keys in this
// order, so a node carries the bits Transformer::forward gives when it is fed the node's root-to-node path token by token, and no stale row of a sibling
// (which need not be finite) meets a weight.  A chain - parent[j] = j - 1 - has anc[t - base] = t - base: the ragged pass, bit for bit, K/V rows included.
// One body serves contiguous slots and f32 page pools (PAGED): only the address of a storage position differs.
// ------------------------------------------------------------------------------------------------
// where storage position s of the row's slot lies: the float offset of its page (PAGED) or slot from k_cache / v_cache, and its place inside (PL positions)
template <bool PAGED> struct TreeSlot {
    const uint32_t* tab; size_t stride; int shift, PL;
    __device__ __forceinline__ TreeSlot(unsigned long long off, const PageView& pv, int seq_len) {
        if constexpr (PAGED) { tab = pv.tab + (size_t)off * pv.per_slot; stride = pv.page_stride; shift = pv.shift; PL = 1 << pv.shift; }
        else { tab = nullptr; stride = (size_t)off; shift = 0; PL = seq_len; }
    }
    __device__ __forceinline__ size_t block(int s) const { if constexpr (PAGED) return (size_t)tab[s >> shift] * stride; else return stride; }
    __device__ __forceinline__ int pin(int s) const { if constexpr (PAGED) return s & (PL - 1); else return s; }
};

// rope_scatter_row / paged_scatter_kernel with two positions a row: the rotation terms are those of the LOGICAL position (rows.pos), the stores go to the
// STORAGE position (TreeRow::spos), looked up in the slot's page row on a paged batch.  q is rotated in place.
template <bool PAGED>
__global__ __launch_bounds__(256) void tree_scatter_kernel(float* qkv, float* k_cache, float* v_cache, const float* rope, const RowView rows, const TreeView tv,
                                                            const PageView pv, int n_heads, int n_kv_heads, int hs, int seq_len, int layer) {
    const int r = blockIdx.x, pos = rows.pos[r], spos = tv.rows[r].spos;
    const TreeSlot<PAGED> slot(rows.off[r], pv, seq_len);
    const int PL = slot.PL, pin = slot.pin(spos);
    const size_t off = slot.block(spos);
    float* row = qkv + (size_t)r * (n_heads + 2 * n_kv_heads) * hs;
    float* k_blk = k_cache + off;
    float* v_blk = v_cache + off;
    const int half = hs / 2, att = n_heads * hs, kv = n_kv_heads * hs;
    for (int i = threadIdx.x; i < (n_heads + n_kv_heads) * half; i += blockDim.x) {
        const int hh = i / half, j = i - hh * half;
        const float2 cs = *reinterpret_cast<const float2*>(rope + ((size_t)pos * half + j) * 2);
        if (hh < n_heads) {
            float* p = row + hh * hs;
            const float2 rq = rope_rotate(p[j], p[j + half], cs.x, cs.y);
            p[j] = rq.x; p[j + half] = rq.y;
        } else {
            const int kvh = hh - n_heads;
            const float* p = row + att + kvh * hs;
            const float2 rk = rope_rotate(p[j], p[j + half], cs.x, cs.y);
            k_store_pair(k_blk + ((size_t)layer * n_kv_heads + kvh) * hs * (size_t)PL, PL, pin, j, half, rk.x, rk.y);
        }
    }
    const float4* v = reinterpret_cast<const float4*>(row + att + kv);
    float4* vd = reinterpret_cast<float4*>(v_blk + ((size_t)layer * PL + pin) * kv);
    for (int i = threadIdx.x; i < kv / 4; i += blockDim.x) vd[i] = v[i];
}

static bool tree_pages_ok(const PageView& pv) { return !pv.tab || (pv.shift >= 6 && pv.per_slot >= 1); }

hipError_t launch_tree_scatter(float* qkv, float* k_cache, float* v_cache, const float* rope, RowView rows, TreeView tv, PageView pv, int n_heads, int n_kv_heads,
                               int hs, int seq_len, int layer, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRunRowsMax || !tv.rows || !tree_pages_ok(pv)) return hipErrorInvalidValue;
    if (pv.tab) hipLaunchKernelGGL(tree_scatter_kernel<true>, dim3(n_rows), dim3(256), 0, s, qkv, k_cache, v_cache, rope, rows, tv, pv, n_heads, n_kv_heads, hs, seq_len, layer);
    else hipLaunchKernelGGL(tree_scatter_kernel<false>, dim3(n_rows), dim3(256), 0, s, qkv, k_cache, v_cache, rope, rows, tv, pv, n_heads, n_kv_heads, hs, seq_len, layer);
    return hipGetLastError();
}

// att_gload with a storage position per tile row: the chunk t0 .. of LOGICAL keys that reaches into the tree, whose rows are neither consecutive in the
// cache nor, on a paged batch, in one page.  Slot geometry, the clamp of the rows past the chunk's last one and the load itself are att_gload's; row_ptr(t)
// is the V row of logical key t at this kv head's columns.
template <int HS, int NF, class RowPtr>
__device__ __forceinline__ void tree_gload(float4 (&rg)[NF], int t0, int T, int CH, RowPtr row_ptr) {
    constexpr int HS4 = HS / 4;
    const int ct = (T - t0) < CH ? (T - t0) : CH, nrows = (ct + 15) & ~15, nf = nrows * HS4;
    const int r0 = (int)threadIdx.x / HS4, c4 = (int)threadIdx.x - r0 * HS4;
#pragma unroll
    for (int i0 = 0; i0 < NF; i0 += 4) {
        if (i0 * kBlock < nf) {                                              // wave-uniform
#pragma unroll
            for (int i = i0; i < i0 + 4 && i < NF; ++i) {
                int row;
                if constexpr (kBlock % HS4 == 0) row = r0 + i * (kBlock / HS4);
                else row = ((int)threadIdx.x + i * kBlock) / HS4;
                const int col4 = (kBlock % HS4 == 0) ? 0 : (((int)threadIdx.x + i * kBlock) - row * HS4 - c4) * 4;
                row = row < ct - 1 ? row : ct - 1;
                rg[i] = ld_f32x4<false>(row_ptr(t0 + row) + c4 * 4 + col4);
            }
        }
    }
}

// one workgroup per (head, row): paged_attention_body's phases over the row's compacted keys
template <int HS, bool GEMMA, bool PAGED>
__global__ __launch_bounds__(kBlock) void tree_attn_kernel(const AttnArgs a, const RowView rows, const TreeView tv, const PageView pv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RS = HS + 4, NF = kAttF4;
    const int r = blockIdx.y, h = blockIdx.x, tid = threadIdx.x;
    const int att_dim = a.n_heads * HS, kv_dim = a.n_kv_heads * HS;
    const float* qrow = a.q + (size_t)r * (att_dim + 2 * kv_dim);
    const int kv_mul = a.n_heads / a.n_kv_heads, kvh = h / kv_mul;
    const int pos = rows.pos[r], base = tv.rows[r].base, T = pos + 1;                    // pos: the LOGICAL position, base + depth
    const uint8_t* anc = tv.rows[r].anc;
    const TreeSlot<PAGED> slot(rows.off[r], pv, a.seq_len);
    const int CH = a.chunk, PL = slot.PL;
    const uint64_t etab = exp2f_tab_lane();
    float* q = reinterpret_cast<float*>(smem);        // the LDS layout is attention_body's (attention_smem)
    float* red = q + 3 * HS;
    float* tile = red + 16;
    float* att = tile + (size_t)(CH + 32) * RS;
    const int nchunks = (T + CH - 1) / CH;
    const size_t k_head = ((size_t)a.layer * a.n_kv_heads + kvh) * HS * (size_t)PL;      // this kv head's K block inside a page / slot
    const size_t v_head = (size_t)a.layer * PL * kv_dim + kvh * HS;                      // this layer's V rows there, at the kv head's columns
    // logical key t -> its storage position: the prefix lies where it is counted, a tree key where its node was stored
    auto stored = [&](int t) __attribute__((always_inline)) { return t < base ? t : base + (int)anc[t - base]; };
    auto key_of = [&](int t) __attribute__((always_inline)) { const int s = stored(t); return a.k_cache + slot.block(s) + k_head + (size_t)slot.pin(s) * 4; };
    auto v_row = [&](int t) __attribute__((always_inline)) { const int s = stored(t); return a.v_cache + slot.block(s) + v_head + (size_t)slot.pin(s) * kv_dim; };
    // the V chunk of logical keys t0 .. : wholly in the prefix it is CH consecutive rows of ONE page (CH divides page_len) - paged_attention_body's load;
    // the one or two chunks that reach into [base, T) gather a row at a time
    auto v_load = [&](float4 (&rg)[NF], int t0) __attribute__((always_inline)) {
        if (t0 + CH <= base) {                                                           // wave-uniform
            const int pin = slot.pin(t0);
            att_gload<HS, NF>(rg, a.v_cache + slot.block(t0) + v_head, pin, pin + (T - t0), CH, kv_dim);
        } else tree_gload<HS, NF>(rg, t0, T, CH, v_row);
    };
    constexpr int KG = HS / 4 <= 32 ? HS / 4 : 16;
    static_assert((HS / 4) % KG == 0, "head size");
    const int tc0 = tid < T ? tid : T - 1;            // lanes past the sequence re-read its last key (no predication)
    const float* kp0 = key_of(tc0);
    f32x4v kk[KG];
    paged_kload<KG>(kk, kp0, 0, PL);
    float4 vreg[NF];
    v_load(vreg, 0);
    for (int j = tid; j < HS; j += kBlock) q[j] = qrow[h * HS + j];
    lds_barrier();

    // ---- scores: one lane per logical t, sequential dot over the head dims
    int wpos = pos;
    if constexpr (GEMMA) { const int wb = a.st->win_base; wpos = wb >= 0 ? wb : pos; }
    const float sqrt_hs = sqrtf((float)HS);
    float lmax = __uint_as_float(0xff800000u);
    auto finish_score = [&](float score, int t) __attribute__((always_inline)) {
        score = score / sqrt_hs;
        if constexpr (GEMMA) score = gemma_cap_window(score, wpos, t);
        if (t < T) { att[t] = score; lmax = fmaxf(lmax, score); }
    };
    finish_score(paged_score_chain<HS, KG>(kk, kp0, q, PL), tid);
    for (int t0 = kBlock; t0 < T; t0 += kBlock) {
        const int t = t0 + tid, tc = t < T ? t : T - 1;
        const float* kp = key_of(tc);
        f32x4v k0[KG];
        paged_kload<KG>(k0, kp, 0, PL);
        finish_score(paged_score_chain<HS, KG>(k0, kp, q, PL), t);
    }
    // ---- softmax: max (order-free), exp, sequential sum, divide
    lmax = wave64_max(lmax);
    if ((tid & 63) == 0) red[tid >> 6] = lmax;
    lds_barrier();
    const float mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    for (int t0 = 0; t0 < T; t0 += kBlock) {
        const int t = t0 + tid;
        const float e = expf_glibc_t(t < T ? att[t] - mx : 0.0f, etab);
        if (t < T) att[t] = e;
    }
    if (tid < 64) att[T + tid] = 0.0f;
    lds_barrier();
    if (tid < 64) {
        float sum = 0.0f;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int left = T - t0;
            sum = wave_serial_sum(sum, att[t0 + tid], left >= 64 ? 4 : (left + 15) >> 4);
        }
        if (tid == 0) red[4] = sum;
    }
    lds_barrier();
    const float sum = red[4];
    for (int t = tid; t < T; t += kBlock) att[t] = att[t] / sum;
    lds_barrier();

    // ---- weighted sum of values: products into the tile, one lane per output dim adds them up sequentially over the logical t
    float o = 0.0f;
    for (int c = 0; c < nchunks; ++c) {
        const int t0 = c * CH, ct = (T - t0) < CH ? (T - t0) : CH;
        att_tstore<HS, NF, true>(vreg, tile, att + t0, t0, T, CH, -1, q);
        lds_barrier();
        if (c + 1 < nchunks) v_load(vreg, t0 + CH);
        if (tid < HS) o = serial_sum16<RS, false>(o, tile + tid, ct);
        lds_barrier();
    }
    if (tid < HS) a.out[(size_t)r * att_dim + h * HS + tid] = o;
}

hipError_t launch_tree_attention(const AttnArgs& a0, RowView rows, TreeView tv, PageView pv, int n_rows, int max_T, hipStream_t s) {
    AttnArgs a = a0;
    a.chunk = 64;                                                          // as launch_paged_attention; 64 divides every page_len
    if (n_rows < 1 || n_rows > kRunRowsMax || max_T < 1 || max_T > a.seq_len || a.chunk * (a.head_size / 4) > kAttF4 * kBlock) return hipErrorInvalidValue;
    if (!tv.rows || !tree_pages_ok(pv)) return hipErrorInvalidValue;
    const size_t smem = attention_smem(a.head_size, a.chunk, max_T);       // (max_T: the deepest row's LOGICAL position + 1)
#define TA(HS_, G_, P_)                                                                                                               \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(tree_attn_kernel<HS_, G_, P_>));                                                  \
        hipLaunchKernelGGL((tree_attn_kernel<HS_, G_, P_>), dim3(a.n_heads, n_rows), dim3(kBlock), smem, s, a, rows, tv, pv);          \
        return hipGetLastError();                                                                                                     \
    }
#define TP(HS_, G_) { if (pv.tab) TA(HS_, G_, true) else TA(HS_, G_, false) }
    if (a.gemma) { if (a.head_size == 256) TP(256, true) return hipErrorInvalidValue; }
    switch (a.head_size) { case 64: TP(64, false) case 96: TP(96, false) case 128: TP(128, false) default: return hipErrorInvalidValue; }
#undef TP
#undef TA
}

// lmrs_batch_accept_path: per entry the K and V rows of every layer move from storage position start + path[j] to start + j, j ascending.  One thread owns
// one 16-byte column group - four dims of one kv head's key ([layer][kv head][hs / 4][positions][4]: the four lie together at every position) or four floats
// of the V row - of one (entry, layer, K-or-V) and walks the path itself, reading path[j] and then writing j.  path is strictly ascending (path[j] >= j), so
// within a column every source lies above every destination written before it: a destination that is an earlier source (path = [1, 2]) is consumed by then.
template <bool PAGED>
__global__ __launch_bounds__(256) void tree_commit_kernel(float* k_cache, float* v_cache, const TreeMove* moves, const PageView pv, int n_layers, int kv_dim, int seq_len) {
    const TreeMove& m = moves[blockIdx.y];
    const int kv4 = kv_dim / 4, per_layer = 2 * kv4;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_layers * per_layer) return;
    const int layer = i / per_layer, c = i - layer * per_layer;
    const bool is_v = c >= kv4;
    const int g = is_v ? c - kv4 : c;
    const TreeSlot<PAGED> slot(m.off, pv, seq_len);
    const int PL = slot.PL, start = m.start, len = m.len;
    float* const blk = is_v ? v_cache : k_cache;
    auto at = [&](int s) __attribute__((always_inline)) {
        const size_t pin = (size_t)slot.pin(s);
        const size_t e = is_v ? ((size_t)layer * PL + pin) * kv_dim + (size_t)g * 4 : (((size_t)layer * kv4 + g) * PL + pin) * 4;
        return reinterpret_cast<float4*>(blk + slot.block(s) + e);
    };
    for (int j = 0; j < len; ++j) {
        const int from = (int)m.path[j];
        if (from == j) continue;
        const float4 v = *at(start + from);
        *at(start + j) = v;
    }
}

hipError_t launch_tree_commit(float* k_cache, float* v_cache, const TreeMove* moves, PageView pv, int n_layers, int kv_dim, int seq_len, int n_moves, hipStream_t s) {
    if (n_moves < 1 || n_moves > kTreeMovesMax || !moves || kv_dim % 4 || !tree_pages_ok(pv)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n_layers * 2 * (kv_dim / 4) + 255) / 256), (unsigned)n_moves);
    if (pv.tab) hipLaunchKernelGGL(tree_commit_kernel<true>, grid, dim3(256), 0, s, k_cache, v_cache, moves, pv, n_layers, kv_dim, seq_len);
    else hipLaunchKernelGGL(tree_commit_kernel<false>, grid, dim3(256), 0, s, k_cache, v_cache, moves, pv, n_layers, kv_dim, seq_len);
    return hipGetLastError();
}
