// ------------------------------------------------------------------------------------------------
// The table passes over PAGED K/V (lmrs_batch_create_paged; included by lmrs_kernels.hip behind lmrs_prefill.inc).  A slot's cache is a row of
// page numbers (PageView, lmrs_kernels.h); a page has the contiguous slot layout with page_len in the place of seq_len - K [layer][kv head][hs / 4]
// [page_len][4], V [layer][page_len][kv_dim] - so position p of a slot lives in page tab[p / page_len] at in-page position p % page_len.  The rows'
// `off` word carries the slot's table row.  Paging moves addresses only: the two kernels below perform rope_scatter_row's and
// attention_body<HS, kAttF4, false, false, GEMMA, true>'s operations in the same order per value, so every output carries the contiguous pass's
// bits.  The table is read at run time: the device-resident loop of lmrs_batch_generate_greedy crosses page edges with no host step.
// ------------------------------------------------------------------------------------------------
// rope_scatter_row with the destination looked up: the rotation terms are those of `pos`, the stores go to in-page position pos % page_len
__global__ __launch_bounds__(256) void paged_scatter_kernel(float* qkv, float* k_pool, float* v_pool, const float* rope, const RowView rows, const PageView pv,
                                                             int n_heads, int n_kv_heads, int hs, int layer) {
    const int r = blockIdx.x, pos = rows.pos[r], PL = 1 << pv.shift, pin = pos & (PL - 1);
    const size_t off = (size_t)pv.tab[(size_t)rows.off[r] * pv.per_slot + (pos >> pv.shift)] * pv.page_stride;
    float* row = qkv + (size_t)r * (n_heads + 2 * n_kv_heads) * hs;
    float* k_page = k_pool + off;
    float* v_page = v_pool + off;
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
            k_store_pair(k_page + ((size_t)layer * n_kv_heads + kvh) * hs * (size_t)PL, PL, pin, j, half, rk.x, rk.y);
        }
    }
    const float4* v = reinterpret_cast<const float4*>(row + att + kv);
    float4* vd = reinterpret_cast<float4*>(v_page + ((size_t)layer * PL + pin) * kv);
    for (int i = threadIdx.x; i < kv / 4; i += blockDim.x) vd[i] = v[i];
}

hipError_t launch_paged_scatter(float* qkv, float* k_pool, float* v_pool, const float* rope, RowView rows, PageView pv, int n_heads, int n_kv_heads, int hs,
                                int layer, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRunRowsMax || !pv.tab || pv.shift < 6 || pv.per_slot < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(paged_scatter_kernel, dim3(n_rows), dim3(256), 0, s, qkv, k_pool, v_pool, rope, rows, pv, n_heads, n_kv_heads, hs, layer);
    return hipGetLastError();
}

// att_kload / att_score_chain with a 64-bit address per lane: kp = this lane's key inside ITS page (dim group 0), the groups page_len * 4 floats apart.
// A 256-key pass may span four pages (and a pool more than 4 GB), so no one buffer descriptor covers it; the loads are plain global 16-byte loads.
// The arithmetic - att_kuse, the batches' order, the opaque asm between them - is att_score_chain's.
template <int NG>
__device__ __forceinline__ void paged_kload(f32x4v (&dst)[NG], const float* kp, int g0, int PL) {
#pragma unroll
    for (int u = 0; u < NG; ++u) dst[u] = *reinterpret_cast<const f32x4v*>(kp + (size_t)(g0 + u) * PL * 4);
}
template <int HS, int NG>
__device__ __forceinline__ float paged_score_chain(f32x4v (&kk)[NG], const float* kp, const float* q, int PL) {
    constexpr int HS4 = HS / 4;
    f32x4v kb[NG];
    float score = 0.0f;
    const float4* q4 = reinterpret_cast<const float4*>(q);
#pragma unroll
    for (int g0 = 0; g0 < HS4; g0 += 2 * NG) {
        if (g0 + NG < HS4) paged_kload<NG>(kb, kp, g0 + NG, PL);
        score = att_kuse<NG>(score, kk, q4, g0);
        asm volatile("" : "+v"(score) : : "memory");
        if (g0 + NG < HS4) {
            if (g0 + 2 * NG < HS4) paged_kload<NG>(kk, kp, g0 + 2 * NG, PL);
            score = att_kuse<NG>(score, kb, q4, g0 + NG);
            asm volatile("" : "+v"(score) : : "memory");
        }
    }
    return score;
}

// attention_body's ROT form (q rotated, every key of the pass already stored) over one slot's page row `tab`
template <int HS, bool GEMMA>
__device__ __forceinline__ void paged_attention_body(const AttnArgs& a, const uint32_t* tab, int shift, size_t page_stride, int h, int pos, char* smem, uint64_t etab) {
    constexpr int RS = HS + 4, NF = kAttF4;
    const int kv_mul = a.n_heads / a.n_kv_heads, kvh = h / kv_mul;
    const int kv_dim = a.n_kv_heads * HS;
    const int T = pos + 1;
    const int tid = threadIdx.x;
    const int CH = a.chunk, PL = 1 << shift;
    float* q = reinterpret_cast<float*>(smem);        // the LDS layout is attention_body's (attention_smem)
    float* red = q + 3 * HS;
    float* tile = red + 16;
    float* att = tile + (size_t)(CH + 32) * RS;
    const int nchunks = (T + CH - 1) / CH;
    const size_t k_head = ((size_t)a.layer * a.n_kv_heads + kvh) * HS * (size_t)PL;      // this kv head's K block inside a page
    const size_t v_head = (size_t)a.layer * PL * kv_dim + kvh * HS;                      // this layer's V rows inside a page, at the kv head's columns
    auto key_of = [&](int t) __attribute__((always_inline)) { return a.k_cache + (size_t)tab[t >> shift] * page_stride + k_head + (size_t)(t & (PL - 1)) * 4; };
    // the V chunk of rows t0 .. : CH divides page_len, so a chunk lies in ONE page - one table lookup a chunk
    auto v_load = [&](float4 (&rg)[NF], int t0) __attribute__((always_inline)) {
        const int pin = t0 & (PL - 1);
        att_gload<HS, NF>(rg, a.v_cache + (size_t)tab[t0 >> shift] * page_stride + v_head, pin, pin + (T - t0), CH, kv_dim);
    };
    constexpr int KG = HS / 4 <= 32 ? HS / 4 : 16;
    static_assert((HS / 4) % KG == 0, "head size");
    const int tc0 = tid < T ? tid : T - 1;            // lanes past the sequence re-read its last key (no predication)
    const float* kp0 = key_of(tc0);
    f32x4v kk[KG];
    paged_kload<KG>(kk, kp0, 0, PL);
    float4 vreg[NF];
    v_load(vreg, 0);
    for (int j = tid; j < HS; j += kBlock) q[j] = a.q[h * HS + j];
    lds_barrier();

    // ---- scores: one lane per t, sequential dot over the head dims
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

    // ---- weighted sum of values: products into the tile, one lane per output dim adds them up sequentially over t
    float o = 0.0f;
    for (int c = 0; c < nchunks; ++c) {
        const int t0 = c * CH, ct = (T - t0) < CH ? (T - t0) : CH;
        att_tstore<HS, NF, true>(vreg, tile, att + t0, t0, T, CH, -1, q);
        lds_barrier();
        if (c + 1 < nchunks) v_load(vreg, t0 + CH);
        if (tid < HS) o = serial_sum16<RS, false>(o, tile + tid, ct);
        lds_barrier();
    }
    if (tid < HS) a.out[h * HS + tid] = o;
}

// one workgroup per (head, row) over a RowView, as attention_runs_kernel: the row's slot is its page row
template <int HS, bool GEMMA>
__global__ __launch_bounds__(kBlock) void paged_attn_kernel(const AttnArgs a0, const RowView rows, const PageView pv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AttnArgs a = a0;
    const int r = blockIdx.y, h = blockIdx.x, att = a.n_heads * HS, kv = a.n_kv_heads * HS;
    a.q = a0.q + (size_t)r * (att + 2 * kv); a.out = a0.out + (size_t)r * att; a.dbg = nullptr;
    const uint64_t etab = exp2f_tab_lane();
    paged_attention_body<HS, GEMMA>(a, pv.tab + (size_t)rows.off[r] * pv.per_slot, pv.shift, pv.page_stride, h, rows.pos[r], smem, etab);
}

hipError_t launch_paged_attention(const AttnArgs& a0, RowView rows, PageView pv, int n_rows, int max_T, hipStream_t s) {
    AttnArgs a = a0;
    a.chunk = 64;                                                          // as launch_attention_runs; 64 divides every page_len
    if (n_rows < 1 || n_rows > kRunRowsMax || max_T < 1 || max_T > a.seq_len || a.chunk * (a.head_size / 4) > kAttF4 * kBlock) return hipErrorInvalidValue;
    if (!pv.tab || pv.shift < 6 || pv.per_slot < 1) return hipErrorInvalidValue;
    const size_t smem = attention_smem(a.head_size, a.chunk, max_T);
#define AP(HS_, G_)                                                                                                                   \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(paged_attn_kernel<HS_, G_>));                                                     \
        hipLaunchKernelGGL((paged_attn_kernel<HS_, G_>), dim3(a.n_heads, n_rows), dim3(kBlock), smem, s, a, rows, pv);                 \
        return hipGetLastError();                                                                                                     \
    }
    if (a.gemma) { if (a.head_size == 256) AP(256, true) return hipErrorInvalidValue; }
    switch (a.head_size) { case 64: AP(64, false) case 96: AP(96, false) case 128: AP(128, false) default: return hipErrorInvalidValue; }
#undef AP
}
