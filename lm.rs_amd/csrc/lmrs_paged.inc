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

// ------------------------------------------------------------------------------------------------
// BLOCK attention over the page table: a prompt chunk of ONE slot - n_tok consecutive rows from pos0 on - through launch_attention_block's three launches
// with the two readers of the K/V cache looked up.  q is rotated and every key and value row of the chunk is in the slot's pages already
// (launch_paged_scatter over the chunk's rows), so the score launch is att_stage's `k_raw == nullptr` form and nothing here stores to a page.
// Both readers walk the key axis in chunks of 64 keys (Gemma's short form: 32) that start at multiples of their length; page_len is a multiple of 64,
// so a chunk or a tile lies in ONE page - one wave-uniform table lookup each.  Past-the-end keys are clamped to the block's last key, as in the
// contiguous kernels, and the table index is formed from the CLAMPED key: the value phase prefetches up to four tiles past the end, whose tile number
// may name an entry past the slot's row (or, for the last slot, past the table).  An entry of a position nobody wrote is page 0, the zero page.
// The sums are att_scores_kernel's / att_scores_wide_kernel's / att_values_kernel's, built from the same helpers in the same order: the same bits.
// qs: floats between query rows (the qkv block: att + 2 kv); tab: the slot's page row; k_pool / v_pool: the K and the V block of page 0.
// ------------------------------------------------------------------------------------------------
struct BlockPages { const uint32_t* tab; int shift; size_t page_stride; int layer; };
template <int HS, int RS, int NK = 64, int NT = 256>
__device__ __forceinline__ void block_paged_stage(float* qt, float* kt, const float* __restrict__ qrows, int qs, const float* __restrict__ k_pool, const BlockPages pg,
                                                  int n_kv_heads, int h, int kvh, int qb, int cb, int bT, int n_tok) {
    constexpr int HS4 = HS / 4;
    const int tid = threadIdx.x, PL = 1 << pg.shift;
    const int kc = cb < bT ? cb : bT - 1;                                     // the chunk's first key, clamped: its page holds every clamped key of the chunk
    const float* kT = k_pool + (size_t)pg.tab[kc >> pg.shift] * pg.page_stride + ((size_t)pg.layer * n_kv_heads + kvh) * HS * (size_t)PL;   // [HS/4][page_len][4]
    for (int f = tid; f < 64 * HS4; f += NT) {
        const int r = f / HS4, c4 = f - r * HS4;
        int qi = qb * kAttQB + r; qi = qi < n_tok ? qi : n_tok - 1;
        *reinterpret_cast<float4*>(qt + r * RS + c4 * 4) = *reinterpret_cast<const float4*>(qrows + (size_t)qi * qs + h * HS + c4 * 4);
        if (NK == 64 || f < NK * HS4) {
            const int g = f / NK, kl = f % NK;
            const int key = cb + kl < bT ? cb + kl : bT - 1;
            *reinterpret_cast<float4*>(kt + kl * RS + g * 4) = *reinterpret_cast<const float4*>(kT + ((size_t)g * PL + (key & (PL - 1))) * 4);
        }
    }
}
template <int HS>
__global__ __launch_bounds__(256) void block_paged_scores_kernel(const float* __restrict__ qrows, int qs, const float* __restrict__ k_pool, const BlockPages pg,
                                                                 float* __restrict__ scratch, int n_heads, int n_kv_heads, int pos0, int n_tok, int Tmax) {
    constexpr int RS = HS + 4, HS4 = HS / 4;
    __shared__ __attribute__((aligned(16))) float qt[64 * RS];
    __shared__ __attribute__((aligned(16))) float kt[64 * RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), qb = gridDim.z - 1 - blockIdx.z, h = blockIdx.x;
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    const int cb = blockIdx.y * 64;
    if (cb >= b.T) return;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul;
    float* S = scratch + ((size_t)h * gridDim.z + qb) * (size_t)Tmax * kAttQB + lane;
    block_paged_stage<HS, RS>(qt, kt, qrows, qs, k_pool, pg, n_kv_heads, h, kvh, qb, cb, b.T, n_tok);
    __syncthreads();
    const int c0 = cb + wave * 16;
    if (c0 >= b.T) return;
    const int nk = b.T - c0 < 16 ? b.T - c0 : 16;
    f32x4v q[HS4];
#pragma unroll
    for (int u = 0; u < HS4; ++u) q[u] = *reinterpret_cast<const f32x4v*>(qt + lane * RS + u * 4);
    const float sqrt_hs = sqrtf((float)HS);
    const float* kv = kt + wave * 16 * RS;
    constexpr int UB = 2;
    static_assert(HS4 % (2 * UB) == 0, "head size");
#pragma unroll 1
    for (int kk = 0; kk < nk; kk += 4) {
        const float* kr = kv + kk * RS;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
        f32x4v ka[4][UB], kb[4][UB];
        att_kread<UB, RS>(ka, kr, 0);
#pragma unroll
        for (int u0 = 0; u0 < HS4; u0 += 2 * UB) {
            att_kread<UB, RS>(kb, kr, u0 + UB);
            att_kdot<UB>(s0, s1, s2, s3, ka, q + u0);
            asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3) : : "memory");
            if (u0 + 2 * UB < HS4) att_kread<UB, RS>(ka, kr, u0 + 2 * UB);
            att_kdot<UB>(s0, s1, s2, s3, kb, q + u0 + UB);
            asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3) : : "memory");
        }
        const float sc[4] = {s0 / sqrt_hs, s1 / sqrt_hs, s2 / sqrt_hs, s3 / sqrt_hs};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (kk + j < nk) S[(size_t)(c0 + kk + j) * kAttQB] = sc[j];
    }
}
// att_scores_wide_kernel (Gemma-2's 256-wide heads: two passes of 128 dims, the soft-cap, the window term) over the pages
template <int HS, int NK, int NT>
__global__ __launch_bounds__(NT) void block_paged_scores_wide_kernel(const float* __restrict__ qrows, int qs, const float* __restrict__ k_pool, const BlockPages pg,
                                                                      float* __restrict__ scratch, const DevState* __restrict__ st, int n_heads, int n_kv_heads,
                                                                      int pos0, int n_tok, int Tmax) {
    constexpr int HP = HS / 2, RS = HS + 4, HP4 = HP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* qt = reinterpret_cast<float*>(smem_raw);              // [64][RS]
    float* kt = qt + 64 * RS;                                    // [NK][RS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), qb = gridDim.z - 1 - blockIdx.z, h = blockIdx.x;
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    constexpr int KW = NK / (NT / 64);
    static_assert(KW % 4 == 0 && KW >= 4 && 64 % NK == 0, "four score chains at a time; a chunk lies in one page");
    const int cb = blockIdx.y * NK;
    if (cb >= b.T) return;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul;
    float* S = scratch + ((size_t)h * gridDim.z + qb) * (size_t)Tmax * kAttQB + lane;
    block_paged_stage<HS, RS, NK, NT>(qt, kt, qrows, qs, k_pool, pg, n_kv_heads, h, kvh, qb, cb, b.T, n_tok);
    __syncthreads();
    const int c0 = cb + wave * KW;
    if (c0 >= b.T) return;
    const int nk = b.T - c0 < KW ? b.T - c0 : KW;
    const float* kv = kt + wave * KW * RS;
    float part[KW];
#pragma unroll
    for (int i = 0; i < KW; ++i) part[i] = 0.0f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        f32x4v q[HP4];
#pragma unroll
        for (int u = 0; u < HP4; ++u) q[u] = *reinterpret_cast<const f32x4v*>(qt + lane * RS + pass * HP + u * 4);
#pragma unroll
        for (int kq = 0; kq < KW / 4; ++kq) {
            if (kq * 4 < nk) {
                const float* kr = kv + kq * 4 * RS + pass * HP;
                float s0 = part[kq * 4 + 0], s1 = part[kq * 4 + 1], s2 = part[kq * 4 + 2], s3 = part[kq * 4 + 3];
                constexpr int UB = 2;
                f32x4v ka[4][UB], kb[4][UB];
                att_kread<UB, RS>(ka, kr, 0);
#pragma unroll
                for (int u0 = 0; u0 < HP4; u0 += 2 * UB) {
                    att_kread<UB, RS>(kb, kr, u0 + UB);
                    att_kdot<UB>(s0, s1, s2, s3, ka, q + u0);
                    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3) : : "memory");
                    if (u0 + 2 * UB < HP4) att_kread<UB, RS>(ka, kr, u0 + 2 * UB);
                    att_kdot<UB>(s0, s1, s2, s3, kb, q + u0 + UB);
                    asm volatile("" : "+v"(s0), "+v"(s1), "+v"(s2), "+v"(s3) : : "memory");
                }
                part[kq * 4 + 0] = s0; part[kq * 4 + 1] = s1; part[kq * 4 + 2] = s2; part[kq * 4 + 3] = s3;
            }
        }
    }
    const float sqrt_hs = sqrtf((float)HS);
    const int wb = st->win_base, wpos = wb >= 0 ? wb : (wb == kWinPerQuery ? b.p : pos0);
#pragma unroll
    for (int i = 0; i < KW; ++i) {
        if (i < nk) {
            const int t = c0 + i;
            S[(size_t)t * kAttQB] = gemma_cap_window(part[i] / sqrt_hs, wpos, t);
        }
    }
}

// att_tile_load with the tile's value rows looked up: vh = v_pool + this layer's and kv head's offset inside a page (the slice's columns included)
template <int NT, int SW, int NS, int NV>
__device__ __forceinline__ void block_paged_tile_load(f32x4v (&rw)[NS], f32x4v (&rv)[NV], const float* Sb, const float* vh, const BlockPages pg, int kv_dim, int t, int T) {
    constexpr int SW4 = SW / 4;
    const int tid = threadIdx.x, k0 = t * 64, PL = 1 << pg.shift;
    const int kc = k0 < T ? k0 : T - 1;                                       // the tile's first key, clamped (a prefetch past the end: the last key's page)
    const float* vb = vh + (size_t)pg.tab[kc >> pg.shift] * pg.page_stride;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int f = tid + j * NT, kl = f >> 4, c4 = f & 15;
        const int key = k0 + kl < T ? k0 + kl : T - 1;
        const f32x4v w4 = *reinterpret_cast<const f32x4v*>(Sb + (size_t)key * kAttQB + c4 * 4);
        rw[j] = k0 + kl < T ? w4 : f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int f = tid + j * NT;
        if (NV * NT == 64 * SW4 || f < 64 * SW4) {
            const int kl = f / SW4, c4 = f - kl * SW4;
            const int key = k0 + kl < T ? k0 + kl : T - 1;
            rv[j] = *reinterpret_cast<const f32x4v*>(vb + (size_t)(key & (PL - 1)) * kv_dim + c4 * 4);
        }
    }
}
template <int HS, int NW, int DW>
__global__ __launch_bounds__(NW * 64) void block_paged_values_kernel(const float* __restrict__ v_pool, const BlockPages pg, const float* __restrict__ scratch,
                                                                     float* __restrict__ out, int n_heads, int n_kv_heads, int pos0, int n_tok, int Tmax) {
    constexpr int NT = NW * 64, SW = NW * DW, NS = 64 * 16 / NT, NV = (16 * SW + NT - 1) / NT;
    static_assert(HS % SW == 0 && DW % 4 == 0 && (64 * 16) % NT == 0, "slice geometry");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);
    constexpr int TILE = 64 * 64 + 64 * SW;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = blockIdx.x, sl = blockIdx.z;
    const int qb = (sl & 1) ? (int)blockIdx.y : (int)(gridDim.y - 1 - blockIdx.y);
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    const int T = b.T, n_tiles = (T + 63) / 64;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul, kv_dim = n_kv_heads * HS, att = n_heads * HS;
    const float* Sb = scratch + ((size_t)h * gridDim.y + qb) * (size_t)Tmax * kAttQB;
    const float* vh = v_pool + ((size_t)pg.layer << pg.shift) * kv_dim + kvh * HS + sl * SW;
    f32x4v rwa[NS], rva[NV], rwb[NS], rvb[NV];
    float acc[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) acc[d] = 0.0f;
    block_paged_tile_load<NT, SW, NS, NV>(rwa, rva, Sb, vh, pg, kv_dim, 0, T);
    att_tile_store<NT, SW, NS, NV>(rwa, rva, sm);
    block_paged_tile_load<NT, SW, NS, NV>(rwa, rva, Sb, vh, pg, kv_dim, 1, T);
    block_paged_tile_load<NT, SW, NS, NV>(rwb, rvb, Sb, vh, pg, kv_dim, 2, T);
    lds_barrier();
    for (int t = 0; t < n_tiles; t += 2) {
        att_tile_compute<HS, DW, SW>(acc, sm, lane, wave, T - t * 64);
        if (t + 1 < n_tiles) att_tile_store<NT, SW, NS, NV>(rwa, rva, sm + TILE);
        block_paged_tile_load<NT, SW, NS, NV>(rwa, rva, Sb, vh, pg, kv_dim, t + 3, T);
        lds_barrier();
        if (t + 1 < n_tiles) {
            att_tile_compute<HS, DW, SW>(acc, sm + TILE, lane, wave, T - (t + 1) * 64);
            if (t + 2 < n_tiles) att_tile_store<NT, SW, NS, NV>(rwb, rvb, sm);
            block_paged_tile_load<NT, SW, NS, NV>(rwb, rvb, Sb, vh, pg, kv_dim, t + 4, T);
            lds_barrier();
        }
    }
    if (b.live) {
        float* ob = out + (size_t)b.i * att + h * HS + sl * SW + wave * DW;
#pragma unroll
        for (int g = 0; g < DW / 4; ++g) *reinterpret_cast<float4*>(ob + g * 4) = make_float4(acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]);
    }
}

// launch_attention_block's choices - softmax in LDS or in memory, Gemma's forms by live64 and by slices - over one slot's page row.  a.q: the rotated qkv
// block (row stride att + 2 kv), a.k_cache / a.v_cache: the pool's K and V block of page 0, a.out [n_tok][att]
hipError_t launch_paged_attention_block(const AttnArgs& a, PageView pv, unsigned table_row, int pos0, int n_tok, float* scratch, int lds_keys, bool long_forms, hipStream_t s) {
    const int T = pos0 + n_tok, nqb = (n_tok + kAttQB - 1) / kAttQB, nch = (T + 63) / 64;
    if (!pv.tab || pv.shift < 6 || pv.per_slot < 1 || n_tok < 1 || pos0 < 0 || T > a.seq_len || ((T - 1) >> pv.shift) >= pv.per_slot) return hipErrorInvalidValue;
    const int qs = (a.n_heads + 2 * a.n_kv_heads) * a.head_size;
    const BlockPages pg{pv.tab + (size_t)table_row * pv.per_slot, pv.shift, pv.page_stride, a.layer};
    const bool in_lds = T <= lds_keys;
    const size_t sm = (kAttSW * 64 + kAttSQ + (in_lds ? (size_t)(T + 48) * kAttSQ : 0)) * sizeof(float);
    allow_big_lds(reinterpret_cast<const void*>(att_softmax_kernel<true>));
    auto softmax = [&]() {
        if (in_lds) hipLaunchKernelGGL(att_softmax_kernel<true>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);
        else hipLaunchKernelGGL(att_softmax_kernel<false>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);
    };
#define PV(HS_, NW_, DW_)                                                                                                             \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(block_paged_values_kernel<HS_, NW_, DW_>));                                       \
        hipLaunchKernelGGL((block_paged_values_kernel<HS_, NW_, DW_>), dim3(a.n_heads, nqb, HS_ / (NW_ * DW_)), dim3(NW_ * 64), 2 * (64 * 64 + 64 * NW_ * DW_) * sizeof(float), s, \
                           (const float*)a.v_cache, pg, (const float*)scratch, a.out, a.n_heads, a.n_kv_heads, pos0, n_tok, T);       \
        return hipGetLastError();                                                                                                     \
    }
#define PB(HS_, NW_, DW_)                                                                                                             \
    {                                                                                                                                 \
        hipLaunchKernelGGL((block_paged_scores_kernel<HS_>), dim3(a.n_heads, nch, nqb), dim3(256), 0, s, a.q, qs, (const float*)a.k_cache, pg, scratch,   \
                           a.n_heads, a.n_kv_heads, pos0, n_tok, T);                                                                  \
        softmax();                                                                                                                    \
        PV(HS_, NW_, DW_)                                                                                                             \
    }
    if (a.gemma) {
        if (a.head_size != 256) return hipErrorInvalidValue;
        int live64 = 0;
        for (int qb = 0; qb < nqb; ++qb) { const int last = qb * kAttQB + kAttQB - 1 < n_tok - 1 ? qb * kAttQB + kAttQB - 1 : n_tok - 1; live64 += (pos0 + last + 1 + 63) / 64; }
        live64 *= a.n_heads;
        if (live64 < 512 && !long_forms) {
            constexpr size_t smem32 = (size_t)(64 + 32) * (256 + 4) * sizeof(float);
            allow_big_lds(reinterpret_cast<const void*>(block_paged_scores_wide_kernel<256, 32, 512>));
            hipLaunchKernelGGL((block_paged_scores_wide_kernel<256, 32, 512>), dim3(a.n_heads, (T + 31) / 32, nqb), dim3(512), smem32, s, a.q, qs, (const float*)a.k_cache, pg,
                               scratch, a.st, a.n_heads, a.n_kv_heads, pos0, n_tok, T);
        } else {
            constexpr size_t wide_smem = (size_t)2 * 64 * (256 + 4) * sizeof(float);
            allow_big_lds(reinterpret_cast<const void*>(block_paged_scores_wide_kernel<256, 64, 256>));
            hipLaunchKernelGGL((block_paged_scores_wide_kernel<256, 64, 256>), dim3(a.n_heads, nch, nqb), dim3(256), wide_smem, s, a.q, qs, (const float*)a.k_cache, pg,
                               scratch, a.st, a.n_heads, a.n_kv_heads, pos0, n_tok, T);
        }
        softmax();
        if (a.n_heads * nqb * 4 < 256 && !long_forms) PV(256, 8, 4)
        PV(256, 8, 8)
    }
    switch (a.head_size) { case 64: PB(64, 8, 4) case 96: PB(96, 4, 12) case 128: PB(128, 8, 8) default: return hipErrorInvalidValue; }
#undef PB
#undef PV
}
