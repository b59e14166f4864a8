// lmrs_prefill.inc — forward_layer over a BATCH of tokens (reference transformer.rs:388-657 with sl > 1, reached through
// fill_kv_cache :672-684): the only dense contractions of the path, on the int8 matrix cores.  Included by lmrs_kernels.hip.
//
// matmul_q8 over sl tokens (functional.rs:173-214) is out[t][r] = sum_g ((isum_g(t, r) as f32) * ws[r][g]) * xs[t][g] with the
// groups added in ascending order.  isum_g is an exact int32 dot product over the group's 128 elements, so it may come from
// any summation order - two v_mfma_i32_16x16x64_i8 per group and 16 x 16 (row, token) tile - while the float combine keeps
// the reference's order per output element: every lane owns 4 weight rows of one token and walks the groups in order.
// Results are therefore bit-identical to the per-token GEMV kernels (and to the reference).
//
// Fragments come straight from global memory: both operands are K-contiguous (weights [o][K], activations [tokens][K]), and
// a 16 x 64 int8 fragment is 16 bytes per lane (row = lane & 15, k-chunk = lane >> 4) - one global_load_dwordx4 each, no LDS.
// A wave keeps one 16-row weight fragment against two or four 16-token fragments; 1 or 4 waves per workgroup (launcher).
typedef int i32x4m __attribute__((ext_vector_type(4)));
typedef float f32x4m __attribute__((ext_vector_type(4)));

// One lane's share of the result: weight rows rq .. rq+3 of token t.
template <int EPI>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& a, int rq, int t, float v0, float v1, float v2, float v3) {
    if constexpr (EPI == EPI_STORE) {
        *reinterpret_cast<float4*>(a.out + (size_t)t * a.o + rq) = make_float4(v0, v1, v2, v3);
    } else if constexpr (EPI == EPI_RESID) {                      // x += ...
        float4* p = reinterpret_cast<float4*>(a.out + (size_t)t * a.o + rq);
        float4 x = *p; x.x = x.x + v0; x.y = x.y + v1; x.z = x.z + v2; x.w = x.w + v3; *p = x;
    } else if constexpr (EPI == EPI_QKV) {                        // q | raw k | v -> cache row pos + t (att_dim, kv_dim multiples of 4)
        const float4 v = make_float4(v0, v1, v2, v3);
        if (rq < a.att_dim) *reinterpret_cast<float4*>(a.out + (size_t)t * a.att_dim + rq) = v;
        else if (rq < a.att_dim + a.kv_dim) *reinterpret_cast<float4*>(a.k_raw + (size_t)t * a.kv_dim + (rq - a.att_dim)) = v;
        else *reinterpret_cast<float4*>(a.v_cache + ((size_t)a.layer * a.seq_len + a.pos0 + t) * a.kv_dim + (rq - a.att_dim - a.kv_dim)) = v;
    } else if constexpr (EPI == EPI_SWIGLU) {                     // rows interleaved: 2i gate, 2i+1 up
        float2 hv; hv.x = swiglu(v0, v1); hv.y = swiglu(v2, v3);
        *reinterpret_cast<float2*>(a.out + (size_t)t * (a.o >> 1) + (rq >> 1)) = hv;
    } else if constexpr (EPI == EPI_GELU) {                       // Gemma
        float2 hv; hv.x = geglu(v0, v1); hv.y = geglu(v2, v3);
        *reinterpret_cast<float2*>(a.out + (size_t)t * (a.o >> 1) + (rq >> 1)) = hv;
    } else if constexpr (EPI == EPI_VQKV) {                       // CLIP q | k | v rows + bias, q / sqrt(head_size)  (vision.rs:349-381)
        const float4 b = *reinterpret_cast<const float4*>(a.bias + rq);
        float4 v = make_float4(v0 + b.x, v1 + b.y, v2 + b.z, v3 + b.w);
        if (rq < a.att_dim) { v.x = v.x / a.qscale; v.y = v.y / a.qscale; v.z = v.z / a.qscale; v.w = v.w / a.qscale; }
        *reinterpret_cast<float4*>(a.out + (size_t)t * a.o + rq) = v;
    } else if constexpr (EPI == EPI_BIAS_RESID) {                 // (acc + bias) + residual                       (:436-466, 540-566)
        const float4 b = *reinterpret_cast<const float4*>(a.bias + rq);
        const float4 x = *reinterpret_cast<const float4*>(a.resid + (size_t)t * a.o + rq);
        float4 v = make_float4(v0 + b.x, v1 + b.y, v2 + b.z, v3 + b.w);
        v.x = v.x + x.x; v.y = v.y + x.y; v.z = v.z + x.z; v.w = v.w + x.w;
        *reinterpret_cast<float4*>(a.out + (size_t)t * a.o + rq) = v;
    } else if constexpr (EPI == EPI_BIAS_QGELU) {                 // QuickGELU(acc + bias)                           (:497-516)
        const float4 b = *reinterpret_cast<const float4*>(a.bias + rq);
        float vv[4] = {v0 + b.x, v1 + b.y, v2 + b.z, v3 + b.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float tq = 1.702f * vv[i]; const float e = expf_glibc(-tq); const float g = 1.0f / (1.0f + e); vv[i] = vv[i] * g; }
        *reinterpret_cast<float4*>(a.out + (size_t)t * a.o + rq) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    } else if constexpr (EPI == EPI_BIAS_GELU || EPI == EPI_BIAS) {  // image projector: (acc + bias) [* 0.5 (1 + tanh_f64(..))]   (processor.rs:279-296, 320-336)
        const float4 b = *reinterpret_cast<const float4*>(a.bias + rq);
        float vv[4] = {v0 + b.x, v1 + b.y, v2 + b.z, v3 + b.w};
        if constexpr (EPI == EPI_BIAS_GELU) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float h = vv[i];
                float cube = 0.044715f * h; cube = cube * h; cube = cube * h;
                const float inner = h + cube;
                const double th = tanh(0.7978845608028654 * (double)inner);
                const float g = 0.5f * (1.0f + (float)th);
                vv[i] = h * g;
            }
        }
        *reinterpret_cast<float4*>(a.out + (size_t)t * a.o + rq) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
}

// Q4: packed-nibble weights ([o][K/2] bytes).  A lane's 16 elements of a 64-element K step are 8 packed bytes = two dwords;
// (w & 0x0F0F0F0F) holds their even elements, (w >> 4 & ...) the odd ones, each made signed (nibble - 8) per byte: the int8
// fragment is [even(w0) | odd(w0) | even(w1) | odd(w1)].  The activations of a Q4 batch are stored as int8 (q - 8) in exactly
// that order within every 8 elements (rows_prologue_kernel), so the two operands still pair element with element.
__device__ __forceinline__ i32x4m q4_fragment(int w0, int w1) {
    return i32x4m{nib_signed((unsigned)w0), nib_signed((unsigned)w0 >> 4), nib_signed((unsigned)w1), nib_signed((unsigned)w1 >> 4)};
}

template <int EPI, int MT, int NTT, int WAVES, bool Q4 = false>
__global__ __launch_bounds__(64 * WAVES) void gemm_q8_kernel(const GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, kb = lane >> 4;
    const int K = a.n, G = K / 128;
    const int WB = Q4 ? K / 2 : K;                               // bytes per weight row
    const int r0 = (blockIdx.x * WAVES + wave) * 16 * MT;        // this wave's 16 * MT weight rows
    const int tb = blockIdx.y * (16 * NTT);                      // this workgroup's token block
    if (r0 >= a.o) return;
    // The group scales of this wave's rows and tokens, staged once in LDS as [g][row] / [g][token]: in the K loop they are
    // LDS reads, so the only loop-carried VMEM results are the fragment registers (loop-carried loaded SCALARS get register
    // copies behind a vmcnt(0) at the back edge, which serialises the prefetch).
    constexpr int NR = 16 * MT, NT = 16 * NTT;
    float* wsl = reinterpret_cast<float*>(smem_raw) + (size_t)wave * G * (NR + NT);   // [G][NR]
    float* xsl = wsl + (size_t)G * NR;                                                // [G][NT]
    static_assert(NR <= 64 && NT <= 64 && 64 % NR == 0 && 64 % NT == 0, "one lane per row / token");
    {   // lane -> (row, phase): a row's scales two at a time (G is even), all loads of a lane independent
        constexpr int PW = 64 / NR, PX = 64 / NT;
        int r = r0 + (lane % NR); r = r < a.o ? r : a.o - 1;
        const float* wsp = a.ws + (size_t)r * G;
#pragma unroll 4
        for (int g = (lane / NR) * 2; g < G; g += 2 * PW) {
            const float2 v = *reinterpret_cast<const float2*>(wsp + g);
            wsl[g * NR + (lane % NR)] = v.x; wsl[(g + 1) * NR + (lane % NR)] = v.y;
        }
        int t = tb + (lane % NT); t = t < a.n_tok ? t : a.n_tok - 1;
        const float* xsp = a.xs + (size_t)t * G;
#pragma unroll 4
        for (int g = (lane / NT) * 2; g < G; g += 2 * PX) {
            const float2 v = *reinterpret_cast<const float2*>(xsp + g);
            xsl[g * NT + (lane % NT)] = v.x; xsl[(g + 1) * NT + (lane % NT)] = v.y;
        }
    }
    const int8_t* wrow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int r = r0 + m * 16; r = r < a.o ? r : a.o - 16;         // a ragged last tile re-does the previous one (o is a multiple of 16)
        wrow[m] = static_cast<const int8_t*>(a.wq) + (size_t)(r + lr) * WB + kb * (Q4 ? 8 : 16);
    }
    const int8_t* xrow[NTT];
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        int t = tb + j * 16 + lr; t = t < a.n_tok ? t : a.n_tok - 1;          // tokens past the batch: a harmless duplicate
        xrow[j] = a.xq + (size_t)t * K + kb * 16;
    }

    f32x4m acc[MT][NTT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int j = 0; j < NTT; ++j) acc[m][j] = f32x4m{0.f, 0.f, 0.f, 0.f};

    struct Frag { i32x4m w0[MT], w1[MT], x0[NTT], x1[NTT]; };
    auto load = [&](Frag& f, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if constexpr (!Q4) {
                f.w0[m] = *reinterpret_cast<const i32x4m*>(wrow[m] + g * 128);
                f.w1[m] = *reinterpret_cast<const i32x4m*>(wrow[m] + g * 128 + 64);
            } else {
                const int2 p0 = *reinterpret_cast<const int2*>(wrow[m] + g * 64), p1 = *reinterpret_cast<const int2*>(wrow[m] + g * 64 + 32);
                f.w0[m] = q4_fragment(p0.x, p0.y);
                f.w1[m] = q4_fragment(p1.x, p1.y);
            }
        }
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            f.x0[j] = *reinterpret_cast<const i32x4m*>(xrow[j] + g * 128);
            f.x1[j] = *reinterpret_cast<const i32x4m*>(xrow[j] + g * 128 + 64);
        }
    };
    auto use = [&](const Frag& f, int g) __attribute__((always_inline)) {
        f32x4m wsv[MT]; float xsv[NTT];
#pragma unroll
        for (int m = 0; m < MT; ++m) wsv[m] = *reinterpret_cast<const f32x4m*>(wsl + g * NR + m * 16 + kb * 4);   // the 4 weight rows this lane holds
#pragma unroll
        for (int j = 0; j < NTT; ++j) xsv[j] = xsl[g * NT + j * 16 + lr];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                i32x4m c = {0, 0, 0, 0};
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(f.w0[m], f.x0[j], c, 0, 0, 0);     // D[row = weight row][col = token]
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(f.w1[m], f.x1[j], c, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float p = (float)c[i] * wsv[m][i];            // (ival as f32) * w.s[..]
                    p = p * xsv[j];                               //   * x.s[..]
                    acc[m][j][i] = acc[m][j][i] + p;              // groups ascending
                }
            }
    };
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the scales are in LDS (each wave reads only what it wrote)
    __builtin_amdgcn_wave_barrier();
    Frag fa, fb;
    load(fa, 0);
    for (int g = 0; g < G; g += 2) {                              // G is even (n is a multiple of 256: checked by the launcher)
        load(fb, g + 1);
        __builtin_amdgcn_sched_barrier(0);                        // keep the next group's loads AHEAD of this group's arithmetic
        use(fa, g);
        __builtin_amdgcn_sched_barrier(0);
        load(fa, g + 2 < G ? g + 2 : g);                          // unconditional (the last one re-loads group g): a load under a branch
        __builtin_amdgcn_sched_barrier(0);                        // makes hipcc wait for ALL outstanding loads at the join, prefetch included
        use(fb, g + 1);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue: this lane holds rows rq .. rq+3 of token tb + j*16 + lr, for each of its MT row tiles
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        if (r0 + m * 16 >= a.o) continue;
        const int rq = r0 + m * 16 + kb * 4;
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            const int t = tb + j * 16 + lr;
            if (t >= a.n_tok) continue;
            gemm_epilogue<EPI>(a, rq, t, acc[m][j][0], acc[m][j][1], acc[m][j][2], acc[m][j][3]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Ring-K variant for the narrow projections at a few hundred tokens (wo / w2 / qkv: a few thousand rows, so only a few hundred
// 32 x 64 output tiles - one WAVE per CU with the kernel above, each walking up to 64 groups alone with one group of loads in
// flight).  Split-K is not available: the reference adds a row's group products in group order and float addition does not
// reassociate.  But only that ADD is ordered - the integer dot products and the two multiplies per element are not.  So four waves
// share one output tile: wave w takes the groups g = w (mod 4) - loads, MFMAs and products run in parallel, four times the bytes
// in flight per CU - and parks its products in LDS; after one barrier per round of four groups every wave owns a QUARTER of the
// tile's elements and adds the four waves' products for them, in group order, to running sums it keeps in registers.
// Same operations in the same order per element.
// ------------------------------------------------------------------------------------------------
template <int EPI, bool Q4 = false>
__global__ __launch_bounds__(256) void gemm_q8_ring_kernel(const GemmArgs a) {
    constexpr int MT = 2, NTT = 4, NR = 16 * MT, NT = 16 * NTT, NTILE = MT * NTT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, kb = lane >> 4;
    const int K = a.n, G = K / 128, GW = G / 4;                  // groups per wave (G % 4 == 0: launcher)
    const int WB = Q4 ? K / 2 : K;
    const int r0 = blockIdx.x * NR, tb = blockIdx.y * NT;
    f32x4m* P = reinterpret_cast<f32x4m*>(smem_raw);             // products of a round: [2 buffers][4 waves][NTILE][64 lanes] f32x4
    constexpr int PBUF = 4 * NTILE * 64;
    float* wsl = reinterpret_cast<float*>(smem_raw + 2 * PBUF * 16) + (size_t)wave * GW * (NR + NT);   // this wave's groups: [GW][NR]
    float* xsl = wsl + (size_t)GW * NR;                                                                //                     [GW][NT]
    {   // group scales of this wave's groups (i -> g = 4 i + wave), one lane per row / token
        int r = r0 + (lane % NR); r = r < a.o ? r : a.o - 1;
        const float* wsp = a.ws + (size_t)r * G;
        for (int i = lane / NR; i < GW; i += 64 / NR) wsl[i * NR + (lane % NR)] = wsp[4 * i + wave];
        int t = tb + (lane % NT); t = t < a.n_tok ? t : a.n_tok - 1;
        const float* xsp = a.xs + (size_t)t * G;
        for (int i = lane / NT; i < GW; i += 64 / NT) xsl[i * NT + (lane % NT)] = xsp[4 * i + wave];
    }
    const int8_t* wrow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int r = r0 + m * 16; r = r < a.o ? r : a.o - 16;
        wrow[m] = static_cast<const int8_t*>(a.wq) + (size_t)(r + lr) * WB + kb * (Q4 ? 8 : 16);
    }
    const int8_t* xrow[NTT];
#pragma unroll
    for (int j = 0; j < NTT; ++j) {
        int t = tb + j * 16 + lr; t = t < a.n_tok ? t : a.n_tok - 1;
        xrow[j] = a.xq + (size_t)t * K + kb * 16;
    }
    struct Frag { i32x4m w0[MT], w1[MT], x0[NTT], x1[NTT]; };
    auto load = [&](Frag& f, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if constexpr (!Q4) {
                f.w0[m] = *reinterpret_cast<const i32x4m*>(wrow[m] + g * 128);
                f.w1[m] = *reinterpret_cast<const i32x4m*>(wrow[m] + g * 128 + 64);
            } else {
                const int2 p0 = *reinterpret_cast<const int2*>(wrow[m] + g * 64), p1 = *reinterpret_cast<const int2*>(wrow[m] + g * 64 + 32);
                f.w0[m] = q4_fragment(p0.x, p0.y);
                f.w1[m] = q4_fragment(p1.x, p1.y);
            }
        }
#pragma unroll
        for (int j = 0; j < NTT; ++j) {
            f.x0[j] = *reinterpret_cast<const i32x4m*>(xrow[j] + g * 128);
            f.x1[j] = *reinterpret_cast<const i32x4m*>(xrow[j] + g * 128 + 64);
        }
    };
    // the products of group 4 i + wave: p[m][j][e] = ((isum as f32) * ws) * xs
    auto products = [&](f32x4m (&p)[MT][NTT], const Frag& f, int i) __attribute__((always_inline)) {
        f32x4m wsv[MT]; float xsv[NTT];
#pragma unroll
        for (int m = 0; m < MT; ++m) wsv[m] = *reinterpret_cast<const f32x4m*>(wsl + i * NR + m * 16 + kb * 4);
#pragma unroll
        for (int j = 0; j < NTT; ++j) xsv[j] = xsl[i * NT + j * 16 + lr];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NTT; ++j) {
                i32x4m c = {0, 0, 0, 0};
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(f.w0[m], f.x0[j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(f.w1[m], f.x1[j], c, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) { float q = (float)c[e] * wsv[m][e]; p[m][j][e] = q * xsv[j]; }
            }
    };
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    Frag fa, fb;
    f32x4m p[MT][NTT];
    constexpr int MINE = NTILE / 4;                              // tiles whose running sums this wave keeps (tile index wave * MINE + q)
    f32x4m acc[MINE];
#pragma unroll
    for (int q = 0; q < MINE; ++q) acc[q] = f32x4m{0.f, 0.f, 0.f, 0.f};
    load(fa, wave);
    for (int i = 0; i < GW; ++i) {
        // prefetch the wave's next group (unconditional: the last one re-loads its own), then this group's MFMAs and products
        const int gn = i + 1 < GW ? 4 * (i + 1) + wave : 4 * i + wave;
        if (i & 1) { load(fa, gn); __builtin_amdgcn_sched_barrier(0); products(p, fb, i); }
        else { load(fb, gn); __builtin_amdgcn_sched_barrier(0); products(p, fa, i); }
        __builtin_amdgcn_sched_barrier(0);
        f32x4m* Pw = P + (i & 1) * PBUF;
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int j = 0; j < NTT; ++j) Pw[(wave * NTILE + m * NTT + j) * 64 + lane] = p[m][j];
        lds_barrier();                                           // LDS only: the prefetched fragments stay in flight
        // (double-buffered: a wave writes round i + 2 only after the barrier of round i + 1, which every wave reaches after its reads of round i)
#pragma unroll
        for (int q = 0; q < MINE; ++q) {
            f32x4m v[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) v[w] = Pw[(w * NTILE + wave * MINE + q) * 64 + lane];
#pragma unroll
            for (int w = 0; w < 4; ++w) {                        // groups 4 i, 4 i + 1, 4 i + 2, 4 i + 3: ascending
                acc[q][0] = acc[q][0] + v[w][0]; acc[q][1] = acc[q][1] + v[w][1]; acc[q][2] = acc[q][2] + v[w][2]; acc[q][3] = acc[q][3] + v[w][3];
            }
        }
    }
    // ---- epilogue: this wave's tiles, straight from its registers
#pragma unroll
    for (int q = 0; q < MINE; ++q) {
        const int tix = wave * MINE + q, m = tix / NTT, j = tix - m * NTT;
        if (r0 + m * 16 >= a.o) continue;
        const int rq = r0 + m * 16 + kb * 4, t = tb + j * 16 + lr;
        if (t >= a.n_tok) continue;
        gemm_epilogue<EPI>(a, rq, t, acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
    }
}

// ------------------------------------------------------------------------------------------------
// LDS-DMA ring kernel (round 3; round 5: any WGM x WGN grid of waves).  A workgroup owns a (16 WM WGM) x (16 WN WGN) output tile - every wave a
// (16 WM) x (16 WN) sub-tile - and walks the K groups through an S-slot LDS ring filled by global_load_lds_dwordx4 (no registers, nothing to wait for at
// issue): S - 1 groups of (TM + TN) x 128 bytes are in flight per CU, one s_barrier per group.
//   * ring slot = [TM weight rows | TN token rows] x 128 bytes + their group scales.  The DMA writes lane i's 16 bytes at
//     base + 16 i, so a row is an unpadded 128-byte line; the 16-byte chunks of row r are stored XOR-swizzled (chunk c at slot
//     c ^ ((r >> 1) & 7), applied on the GLOBAL address of the load): a fragment read - 16 rows, one chunk each - touches 16
//     different bank groups.
//   * per group: wait for this wave's loads of the group (counted vmcnt), barrier (everybody's have landed, everybody is done
//     with the slot that is refilled next), issue the loads of group g + S - 1, then 2 MFMAs per tile; the float combine of a tile
//     (`(isum as f32) * ws * xs`, added in group order: the reference's order per element, bit-identical to the GEMV kernels) follows the
//     MFMAs of the next one in the source (hipcc issues a group's MFMAs as one block and its combine as another whatever the source says).
// What bounds it (round 5, tools/ubench/gemmpipe.hip: 60 variants, an ablation and a PMC run - profiles/r5_ubench_gemm_*.txt): one group iteration of a
// 256 x 128 tile takes a CU 1.44 us where its 256 MFMAs need 0.50 - fragment reads + MFMAs 0.81 even without a barrier, the barrier 0.16, the combine
// 0.31, the loads 0.16 - and none of: register-staged loads, three slots with the next group's fragments prefetched, an MFMA / combine interleave forced
// with scheduling group barriers, phase-shifted waves, the int -> float conversion folded into the MFMA's accumulator, split MFMA pairs - moved it.  What
// does is bytes and iterations per output: the biggest tile that still gives most CUs a workgroup (launch_gemm_q8_ring).
// Workgroups that share weight rows are placed on one XCD (block b runs on XCD b % 8): a weight tile crosses HBM once per XCD.
// ------------------------------------------------------------------------------------------------
// Q4 (packed-nibble weights, round 5): a weight row of a group is 64 bytes - 16 rows per 1-KiB wave-load, the four 16-byte chunks of row r stored at
// c ^ ((r >> 2) & 3) (the 8-byte fragment reads of rows r, r + 4, r + 8, r + 12 would share banks otherwise) - and a lane unpacks its 8 packed bytes to the 16
// signed int8 of an MFMA operand after the LDS read (q4_fragment, as the direct kernel does after its global read); the token rows are the int8 (q - 8)
// rows rows_prologue_kernel writes for Q4, in the matching even / odd order.
constexpr bool dma_quad_scales(int tm, int tn) { return tm * tn >= 8192; }   // (measured: the four-wave 64 x 32 / 32 x 32 tiles and the 64 x 64 tile lose 6-10 % with quads - four 4-byte LDS reads and the quad bookkeeping in a short iteration -, the bigger tiles gain as much)
constexpr int dma_scale_quads(int slot, int scq) { return (160 * 1024 - 2 * scq - 1024) / slot >= 6 ? 3 : 2; }   // (a ring of S <= 5 groups needs two quads: 4 x 2 - S >= 3)
template <int EPI, int WM, int WN, int WGM, int WGN, bool Q4 = false, bool QSEL = true>      // QSEL false: scales one group at a time whatever the tile (transposed scale layouts)
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_q8_dma_kernel(const GemmArgs a, const int n_rt, const int n_tt) {
    constexpr int NW = WGM * WGN, TM = 16 * WM * WGM, TN = 16 * WN * WGN, ROWS = TM + TN;
    constexpr int WROWB = Q4 ? 64 : 128;                         // bytes of a weight row per group
    constexpr int WLW = TM * WROWB / 1024, WLT = TN / 8;         // 1-KiB wave-loads per group: weight rows, token rows
    constexpr int NL = (WLW + WLT) / NW;                         // ... per wave
    constexpr int NSW = (ROWS + 63) / 64;                        // waves that fetch 64 group scales each
    constexpr int DATA = TM * WROWB + TN * 128;
    constexpr bool QS = QSEL && dma_quad_scales(TM, TN);                 // group scales four groups at a time (the bigger tiles) or one (the small ones)
    constexpr int SLOT = QS ? DATA : DATA + NSW * 256 + 256;     // bytes of a ring slot: the rows of one group [, their group scales, a dump line]
    // Group scales (round 6): FOUR groups of a row per fetch.  A 4-byte scale per row and group put every row's scale line on the CU's address path once per
    // group - as many line requests as the rows' data themselves (timing-only ablation, every lane's scale from one line: fill_kv_cache(512) 2.87 -> 2.70 ms,
    // Llama-3.2-3B 7.34 -> 6.79).  Now one 16-byte DMA per row and FOUR groups into a ring of three quads, [row][4 groups]; a quad is fetched with its first group.
    constexpr int SCQ = NSW * 1024;                              // bytes of a quad slot (64 rows x 16 bytes per fetching wave)
    constexpr int SQN = dma_scale_quads(SLOT, SCQ);              // quads buffered: two for the short rings of the big tiles, three otherwise
    constexpr int SCALES = QS ? SQN * SCQ + 1024 : 0;            // ... + a dump piece (waves without scales to fetch)
    constexpr int S = (160 * 1024 - SCALES) / SLOT >= 8 ? 8 : (160 * 1024 - SCALES) / SLOT;
    static_assert(!QS || 4 * SQN - S >= 3, "a quad's slot is refilled only after its last group has been consumed");
    static_assert((WLW + WLT) % NW == 0 && ROWS <= 64 * NW, "whole wave-loads per wave; one scale per lane");
    static_assert(S >= 3 && (S - 2) * (NL + 1) <= 63, "ring depth vs the 6-bit vmcnt");
    extern __shared__ __attribute__((aligned(16))) char ring[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave / WGN, wn = wave % WGN;
    const int lr = lane & 15, kb = lane >> 4;
    const int K = a.n, G = K / 128;
    // block -> (row tile, token tile): the 8 XCDs take the row tiles round robin, each XCD runs all token tiles of its row tiles
    int rt, tt;
    {
        const int b = blockIdx.x, x = b & 7, j = b >> 3, per = (n_rt + 7) / 8;     // row tiles per XCD (padded: the grid is 8 * per * n_tt)
        rt = x + 8 * (j / n_tt); tt = j % n_tt;
        if (j / n_tt >= per || rt >= n_rt) return;
    }
    const int r_base = rt * TM, t_base = tt * TN;
    // ---- DMA sources: wave-load wl = wave * NL + q of the slot (weight rows first: 8 rows per wave-load, 16 for Q4; then the token rows, 8 per wave-load)
    const int8_t* src[NL]; int gstep[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int wl = wave * NL + q;
        if (wl < WLW) {
            int row, c;
            if constexpr (Q4) { row = 16 * wl + (lane >> 2); c = (lane & 3) ^ ((row >> 2) & 3); }
            else { row = 8 * wl + (lane >> 3); c = (lane & 7) ^ ((row >> 1) & 7); }
            int r = r_base + row; r = r < a.o ? r : a.o - 1;
            src[q] = static_cast<const int8_t*>(a.wq) + (size_t)r * (Q4 ? K / 2 : K) + c * 16; gstep[q] = WROWB;
        } else {
            const int row = 8 * (wl - WLW) + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
            int t = t_base + row; t = t < a.n_tok ? t : a.n_tok - 1;
            src[q] = a.xq + (size_t)t * K + c * 16; gstep[q] = 128;
        }
    }
    // group scales: lane i of wave w fetches scale number 64 w + i of the slot's ROWS scales (4-byte DMA: lane i lands at base + 4 i)
    const float* ssrc; int sstep = 1;                            // this lane's scale of group g: ssrc[g * sstep] (a transposed layout: sstep = its leading dimension)
    {
        int i = wave * 64 + lane; i = i < ROWS ? i : ROWS - 1;
        if (i < TM) { int r = r_base + i; r = r < a.o ? r : a.o - 1; if (!QS && a.ws_ld) { ssrc = a.ws + r; sstep = a.ws_ld; } else ssrc = a.ws + (size_t)r * G; }
        else { int t = t_base + i - TM; t = t < a.n_tok ? t : a.n_tok - 1; if (!QS && a.xs_ld) { ssrc = a.xs + t; sstep = a.xs_ld; } else ssrc = a.xs + (size_t)t * G; }
    }
    char* const scq = ring + S * SLOT;                           // the scale quads
    auto issue = [&](int g, int sl) __attribute__((always_inline)) {
        char* base = ring + sl * SLOT;
#pragma unroll
        for (int q = 0; q < NL; ++q)
            __builtin_amdgcn_global_load_lds((const LMRS_GLOBAL void*)(src[q] + (size_t)g * gstep[q]),
                                             (__attribute__((address_space(3))) void*)(base + (wave * NL + q) * 1024), 16, 0, 0);
        if constexpr (!QS) {
            const int sw = wave < NSW ? wave : NSW;                                    // (surplus waves: the dump line - every wave issues the same number of loads)
            __builtin_amdgcn_global_load_lds((const LMRS_GLOBAL void*)(ssrc + (size_t)g * sstep), (__attribute__((address_space(3))) void*)(base + DATA + sw * 256), 4, 0, 0);
        } else if ((g & 3) == 0) {                                                     // (wave-uniform) the quad of groups g .. g + 3; a K whose last quad is short re-reads from G - 4
            const int q = g >> 2, gb = g + 4 <= G ? g : G - 4;
            char* dst = wave < NSW ? scq + (q % SQN) * SCQ + wave * 1024 : scq + SQN * SCQ;      // (surplus waves: the dump piece - every wave issues the same number of loads)
            __builtin_amdgcn_global_load_lds((const LMRS_GLOBAL void*)(ssrc + gb), (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
    };
    f32x4m acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[m][j] = f32x4m{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < S - 1; ++g) issue(g < G ? g : G - 1, g);               // (short K: the surplus slots re-load the last group)
    for (int g = 0; g < G; ++g) {
        // this wave's loads of group g have landed when at most the S - 2 younger groups' are outstanding
        // ... and its own fragment reads of group g - 1 are complete (lgkmcnt(0): free, the MFMAs that took them have been issued) before
        // the barrier behind which slot (g - 1) % S is refilled
        // (only the row loads are counted: the scale quads among the younger loads - none in the tail, where the surplus issues re-load the last group - make
        //  the wait a 16-byte load or two stricter than needed, never laxer; group g's own quad is older than all of them)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((S - 2) * (QS ? NL : NL + 1)) : "memory");
        __builtin_amdgcn_s_barrier();
        { const int gn = g + S - 1; issue(gn < G ? gn : G - 1, gn % S); }      // unconditional (uniform vmcnt accounting); slot (g - 1) % S: everybody is past it
        const char* base = ring + (g % S) * SLOT;
        const char* As = base; const char* Bs = base + TM * WROWB;
        const int g4 = g & ~3, gq = g - (g4 + 4 <= G ? g4 : G - 4);                   // index of group g inside its quad (a short last quad was fetched from G - 4)
        const float* sc = QS ? reinterpret_cast<const float*>(scq + ((g >> 2) % SQN) * SCQ) + gq : reinterpret_cast<const float*>(base + DATA);
        i32x4m a0[WM], a1[WM], b0[WN], b1[WN]; f32x4m wsv[WM]; float xsv[WN];
#pragma unroll
        for (int m = 0; m < WM; ++m) {
            const int row = wm * 16 * WM + m * 16 + lr;
            if constexpr (Q4) {
                const int sw = (row >> 2) & 3, half = (kb & 1) * 8;
                const int2 p0 = *reinterpret_cast<const int2*>(As + row * 64 + (((kb >> 1) ^ sw) << 4) + half);
                const int2 p1 = *reinterpret_cast<const int2*>(As + row * 64 + (((2 + (kb >> 1)) ^ sw) << 4) + half);
                a0[m] = q4_fragment(p0.x, p0.y); a1[m] = q4_fragment(p1.x, p1.y);
            } else {
                const int sw = (row >> 1) & 7;
                a0[m] = *reinterpret_cast<const i32x4m*>(As + row * 128 + ((kb ^ sw) << 4));
                a1[m] = *reinterpret_cast<const i32x4m*>(As + row * 128 + (((kb + 4) ^ sw) << 4));
            }
            if constexpr (QS) { const float* s4 = sc + (wm * 16 * WM + m * 16 + kb * 4) * 4; wsv[m] = f32x4m{s4[0], s4[4], s4[8], s4[12]}; }
            else wsv[m] = *reinterpret_cast<const f32x4m*>(sc + wm * 16 * WM + m * 16 + kb * 4);
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int row = wn * 16 * WN + j * 16 + lr, sw = (row >> 1) & 7;
            b0[j] = *reinterpret_cast<const i32x4m*>(Bs + row * 128 + ((kb ^ sw) << 4));
            b1[j] = *reinterpret_cast<const i32x4m*>(Bs + row * 128 + (((kb + 4) ^ sw) << 4));
            xsv[j] = QS ? sc[(TM + wn * 16 * WN + j * 16 + lr) * 4] : sc[TM + wn * 16 * WN + j * 16 + lr];
        }
        // MFMAs of tile i + 1 ahead of the float combine of tile i
        i32x4m cprev;
        {
            i32x4m c = {0, 0, 0, 0};
            c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0[0], b0[0], c, 0, 0, 0);
            cprev = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1[0], b1[0], c, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < WM * WN; ++i) {
            const int m = i / WN, j = i % WN;
            i32x4m cnext = {0, 0, 0, 0};
            if (i + 1 < WM * WN) {
                const int m2 = (i + 1) / WN, j2 = (i + 1) % WN;
                cnext = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0[m2], b0[j2], cnext, 0, 0, 0);
                cnext = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1[m2], b1[j2], cnext, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float p = (float)cprev[e] * wsv[m][e];            // (ival as f32) * w.s[..]
                p = p * xsv[j];                                   //   * x.s[..]
                acc[m][j][e] = acc[m][j][e] + p;                  // groups ascending
            }
            cprev = cnext;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // (the surplus re-loads of the tail: nothing may still be writing LDS at exit)
    if constexpr (EPI == EPI_SWIGLU_Q || EPI == EPI_GELU_Q) {
        // Round 6: the hidden vector never exists in f32.  A 256-row tile (gate / up interleaved) holds 128 values of h per token = exactly one group of the
        // NEXT matmul's activation quantiser (quantization.rs:44-67; transformer.rs:630): maximum over the tile's four row quarters (waves wm, through LDS)
        // and the lane's row quads (kb), the scale max / 127, the rounded quotients - written as int8 + scale where rows_prologue_kernel<.., 0> would
        // have put them.  Same arithmetic as vec_quantize_q8: the candidate by reciprocal, the reference's division for every value near a rounding boundary
        // and for groups whose maximum is zero / denormal / huge.
        static_assert(TM == 256 && !Q4, "one quantisation group of h per token and tile");
        float hv[WM][WN][2], amax[WN];
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            amax[j] = 0.0f;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                if constexpr (EPI == EPI_SWIGLU_Q) { hv[m][j][0] = swiglu(acc[m][j][0], acc[m][j][1]); hv[m][j][1] = swiglu(acc[m][j][2], acc[m][j][3]); }
                else { hv[m][j][0] = geglu(acc[m][j][0], acc[m][j][1]); hv[m][j][1] = geglu(acc[m][j][2], acc[m][j][3]); }
                amax[j] = absmax4(make_float4(hv[m][j][0], hv[m][j][1], 0.0f, 0.0f), amax[j]);
            }
            amax[j] = fmaxf(amax[j], __shfl_xor(amax[j], 16));
            amax[j] = fmaxf(amax[j], __shfl_xor(amax[j], 32));
        }
        __syncthreads();                                          // every wave is past its last fragment reads: the ring is free
        float* red = reinterpret_cast<float*>(ring);              // [WGM][TN]
        if (kb == 0) {
#pragma unroll
            for (int j = 0; j < WN; ++j) red[wm * TN + wn * 16 * WN + j * 16 + lr] = amax[j];
        }
        __syncthreads();
        const int G_out = a.o / 256;                              // groups of h per token
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int tl = wn * 16 * WN + j * 16 + lr, t = t_base + tl;
            float mg = red[tl];
#pragma unroll
            for (int w = 1; w < WGM; ++w) mg = fmaxf(mg, red[w * TN + tl]);
            const bool sane = quant_group_sane(mg);
            const float sc = sane ? div127_sane(mg) : mg / 127.0f;
            const float inv = __builtin_amdgcn_rcpf(sc);
            if (t >= a.n_tok) continue;
            int8_t* dst = a.hq + (size_t)t * (a.o >> 1) + rt * 128 + wm * 8 * WM + kb * 2;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                int q[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    float d;
                    q[i] = quant_q8_cand(hv[m][j][i], inv, d);
                    if (!sane || !(fabsf(d) <= kQuantDevMax)) q[i] = quant_q8(hv[m][j][i], sc);
                }
                *reinterpret_cast<unsigned short*>(dst + m * 8) = (unsigned short)((q[0] & 0xff) | ((q[1] & 0xff) << 8));
            }
            if (wm == 0 && kb == 0) { if (a.hs_ld) a.hs[(size_t)rt * a.hs_ld + t] = sc; else a.hs[(size_t)t * G_out + rt] = sc; }
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < WM; ++m) {
        const int rq = r_base + wm * 16 * WM + m * 16 + kb * 4;
        if (rq >= a.o) continue;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int t = t_base + wn * 16 * WN + j * 16 + lr;
            if (t >= a.n_tok) continue;
            gemm_epilogue<EPI>(a, rq, t, acc[m][j][0], acc[m][j][1], acc[m][j][2], acc[m][j][3]);
        }
    }
}
template <int EPI, int WM, int WN, int WGM, int WGN, bool Q4, bool QSEL>
static hipError_t launch_gemm_q8_dma_sel(const GemmArgs& a, hipStream_t s) {
    constexpr int NW = WGM * WGN, TM = 16 * WM * WGM, TN = 16 * WN * WGN, ROWS = TM + TN, NSW = (ROWS + 63) / 64;
    constexpr bool QS = QSEL && dma_quad_scales(TM, TN);
    constexpr int DATA = TM * (Q4 ? 64 : 128) + TN * 128, SLOT = QS ? DATA : DATA + NSW * 256 + 256, SCALES = QS ? dma_scale_quads(SLOT, NSW * 1024) * NSW * 1024 + 1024 : 0;
    constexpr int S = (160 * 1024 - SCALES) / SLOT >= 8 ? 8 : (160 * 1024 - SCALES) / SLOT;
    const int n_rt = (a.o + TM - 1) / TM, n_tt = (a.n_tok + TN - 1) / TN, per = (n_rt + 7) / 8;
    allow_big_lds(reinterpret_cast<const void*>(gemm_q8_dma_kernel<EPI, WM, WN, WGM, WGN, Q4, QSEL>));
    hipLaunchKernelGGL((gemm_q8_dma_kernel<EPI, WM, WN, WGM, WGN, Q4, QSEL>), dim3(8 * per * n_tt), dim3(64 * NW), (size_t)S * SLOT + SCALES, s, a, n_rt, n_tt);
    return hipGetLastError();
}
template <int EPI, int WM, int WN, int WGM, int WGN, bool Q4 = false>
static hipError_t launch_gemm_q8_dma(const GemmArgs& a, hipStream_t s) {
    // (transposed scale layouts - the text models' layers - need no quads: a group's scales of 64 rows are two lines already; the quads stay for the row-major
    //  callers: the image tower, the projector, the op-level entry points)
    if constexpr (dma_quad_scales(16 * WM * WGM, 16 * WN * WGN)) { if (a.ws_ld || a.xs_ld) return launch_gemm_q8_dma_sel<EPI, WM, WN, WGM, WGN, Q4, false>(a, s); }
    return launch_gemm_q8_dma_sel<EPI, WM, WN, WGM, WGN, Q4, true>(a, s);
}
// ------------------------------------------------------------------------------------------------
// Q4_0, small tiles (round 6): the ring kernel above fetches a weight row's 64 bytes of ONE group per DMA piece - 16 rows x half a cache line - so every line
// of the packed weights crosses the CU's address path twice (once per group) and a Q4_0 tile, with two thirds of a Q8_0 tile's bytes, takes a third LONGER per
// group (64 x 32: 0.43 against 0.33 us).  Here a ring slot is a PAIR of groups: a weight piece is 8 rows x 128 bytes = whole lines (the layout and the XOR
// swizzle of the Q8_0 tile, the row's 128 bytes being groups 2p | 2p + 1), the token rows of the two groups follow as two blocks, one wait and one barrier
// per pair.  A column of WGM waves, each 16 rows against all 16 WN tokens (a packed row is unpacked by one wave).  Same integer sums, same float combine per
// element in group order: bit-identical.
// ------------------------------------------------------------------------------------------------
template <int EPI, int WN, int WGM, int SCAP = 4>
__global__ __launch_bounds__(64 * WGM) void gemm_q4_pair_kernel(const GemmArgs a, const int n_rt, const int n_tt) {
    constexpr int NW = WGM, TM = 16 * WGM, TN = 16 * WN, ROWS = TM + TN;
    constexpr int WLW = TM / 8, WLT1 = TN / 8, WLT = 2 * WLT1;    // 1-KiB wave-loads per PAIR of groups: weight rows (8 rows x 128 B), token rows (8 rows x 128 B, per group)
    constexpr int NL = (WLW + WLT) / NW;                         // ... per wave
    constexpr int NSW = (ROWS + 63) / 64;                        // waves that fetch 64 group scales each (twice: one group each)
    constexpr int DATA = TM * 128 + 2 * TN * 128;
    constexpr int SLOT = DATA + 2 * NSW * 256 + 256;             // rows, the two groups' scales, a dump line
    constexpr int S = (160 * 1024) / SLOT >= SCAP ? SCAP : (160 * 1024) / SLOT;      // (at most SCAP pairs: the small tiles live on two co-resident workgroups per CU)
    static_assert((WLW + WLT) % NW == 0 && ROWS <= 64 * NW && S >= 2 && (S - 2) * (NL + 2) <= 63, "whole wave-loads per wave; one scale per lane; ring depth");
    extern __shared__ __attribute__((aligned(16))) char ring[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, kb = lane >> 4;
    const int K = a.n, G = K / 128, P = G / 2;                   // (K is a multiple of 256: whole pairs)
    int rt, tt;
    {
        const int b = blockIdx.x, x = b & 7, j = b >> 3, per = (n_rt + 7) / 8;
        rt = x + 8 * (j / n_tt); tt = j % n_tt;
        if (j / n_tt >= per || rt >= n_rt) return;
    }
    const int r_base = rt * TM, t_base = tt * TN;
    const int8_t* src[NL]; int dsto[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int wl = wave * NL + q;
        if (wl < WLW) {                                          // weight rows 8 wl ..: the row's 128 bytes of the pair, chunks XOR-swizzled
            const int row = 8 * wl + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
            int r = r_base + row; r = r < a.o ? r : a.o - 1;
            src[q] = static_cast<const int8_t*>(a.wq) + (size_t)r * (K / 2) + c * 16; dsto[q] = wl * 1024;
        } else {                                                 // token rows of group u of the pair
            const int tw = wl - WLW, u = tw / WLT1, row = 8 * (tw - u * WLT1) + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
            int t = t_base + row; t = t < a.n_tok ? t : a.n_tok - 1;
            src[q] = a.xq + (size_t)t * K + c * 16 + u * 128; dsto[q] = TM * 128 + u * TN * 128 + (tw - u * WLT1) * 1024;
        }
    }
    const float* ssrc; int sstep = 1;                            // this lane's scale of group g: ssrc[g * sstep]
    {
        int i = wave * 64 + lane; i = i < ROWS ? i : ROWS - 1;
        if (i < TM) { int r = r_base + i; r = r < a.o ? r : a.o - 1; if (a.ws_ld) { ssrc = a.ws + r; sstep = a.ws_ld; } else ssrc = a.ws + (size_t)r * G; }
        else { int t = t_base + i - TM; t = t < a.n_tok ? t : a.n_tok - 1; if (a.xs_ld) { ssrc = a.xs + t; sstep = a.xs_ld; } else ssrc = a.xs + (size_t)t * G; }
    }
    auto issue = [&](int p, int sl) __attribute__((always_inline)) {
        char* base = ring + sl * SLOT;
#pragma unroll
        for (int q = 0; q < NL; ++q)
            __builtin_amdgcn_global_load_lds((const LMRS_GLOBAL void*)(src[q] + (size_t)p * (wave * NL + q < WLW ? 128 : 256)),
                                             (__attribute__((address_space(3))) void*)(base + dsto[q]), 16, 0, 0);
        const int sw = wave < NSW ? wave : NSW;                  // (surplus waves: the dump line - every wave issues the same number of loads)
        __builtin_amdgcn_global_load_lds((const LMRS_GLOBAL void*)(ssrc + (size_t)(2 * p) * sstep),
                                         (__attribute__((address_space(3))) void*)(base + DATA + (sw < NSW ? sw * 256 : 2 * NSW * 256)), 4, 0, 0);
        __builtin_amdgcn_global_load_lds((const LMRS_GLOBAL void*)(ssrc + (size_t)(2 * p + 1) * sstep),
                                         (__attribute__((address_space(3))) void*)(base + DATA + (sw < NSW ? (NSW + sw) * 256 : 2 * NSW * 256)), 4, 0, 0);
    };
    f32x4m acc[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) acc[j] = f32x4m{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < S - 1; ++p) issue(p < P ? p : P - 1, p);
    for (int p = 0; p < P; ++p) {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((S - 2) * (NL + 2)) : "memory");
        __builtin_amdgcn_s_barrier();
        { const int pn = p + S - 1; issue(pn < P ? pn : P - 1, pn % S); }
        const char* base = ring + (p % S) * SLOT;
        const int row = wave * 16 + lr, sw = (row >> 1) & 7, half = (kb & 1) * 8;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const char* Bs = base + TM * 128 + u * TN * 128;
            const float* sc = reinterpret_cast<const float*>(base + DATA) + u * NSW * 64;
            const int2 p0 = *reinterpret_cast<const int2*>(base + row * 128 + (((u * 4 + (kb >> 1)) ^ sw) << 4) + half);
            const int2 p1 = *reinterpret_cast<const int2*>(base + row * 128 + (((u * 4 + 2 + (kb >> 1)) ^ sw) << 4) + half);
            const i32x4m a0 = q4_fragment(p0.x, p0.y), a1 = q4_fragment(p1.x, p1.y);
            const f32x4m wsv = *reinterpret_cast<const f32x4m*>(sc + wave * 16 + kb * 4);
            i32x4m b0[WN], b1[WN]; float xsv[WN];
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int trow = j * 16 + lr, tsw = (trow >> 1) & 7;
                b0[j] = *reinterpret_cast<const i32x4m*>(Bs + trow * 128 + ((kb ^ tsw) << 4));
                b1[j] = *reinterpret_cast<const i32x4m*>(Bs + trow * 128 + (((kb + 4) ^ tsw) << 4));
                xsv[j] = sc[TM + j * 16 + lr];
            }
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                i32x4m c = {0, 0, 0, 0};
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0[j], c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1[j], c, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pr = (float)c[e] * wsv[e];               // (ival as f32) * w.s[..]
                    pr = pr * xsv[j];                              //   * x.s[..]
                    acc[j][e] = acc[j][e] + pr;                    // groups ascending
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int rq = r_base + wave * 16 + kb * 4;
    if (rq < a.o) {
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int t = t_base + j * 16 + lr;
            if (t >= a.n_tok) continue;
            gemm_epilogue<EPI>(a, rq, t, acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        }
    }
}
template <int EPI, int WN, int WGM, int SCAP = 4>
static hipError_t launch_gemm_q4_pair(const GemmArgs& a, hipStream_t s) {
    constexpr int TM = 16 * WGM, TN = 16 * WN, NSW = (TM + TN + 63) / 64, SLOT = TM * 128 + 2 * TN * 128 + 2 * NSW * 256 + 256, S = (160 * 1024) / SLOT >= SCAP ? SCAP : (160 * 1024) / SLOT;
    const int n_rt = (a.o + TM - 1) / TM, n_tt = (a.n_tok + TN - 1) / TN, per = (n_rt + 7) / 8;
    allow_big_lds(reinterpret_cast<const void*>(gemm_q4_pair_kernel<EPI, WN, WGM, SCAP>));
    hipLaunchKernelGGL((gemm_q4_pair_kernel<EPI, WN, WGM, SCAP>), dim3(8 * per * n_tt), dim3(64 * WGM), (size_t)S * SLOT, s, a, n_rt, n_tt);
    return hipGetLastError();
}
// The ring kernel's tile by shape (tools/ubench/gemmpipe.hip, profiles/r5_ubench_gemm_tiles_dma.txt): what bounds every variant is the CU's
// own group iteration, so the choice is between bigger tiles (more work per iteration) and whole rounds of workgroups over the 256 CUs:
// 256 x 128 (8 waves of 64 x 64), 128 x 128 (8 waves of 32 x 64), 128 x 64 (8 waves of 32 x 32), 96 x 64 (4 waves), 64 x 64 (8 waves of 32 x 16; Q4_0: 4 waves), 64 x 32 and 32 x 32 (4 waves).
// The tile the ring kernel runs a launch with (host only; also behind lmrs_debug_gemm_tile so that the table of DESIGN.md section 4.1 is a test).
// MI355X-ONLY MODEL: the 256 CUs and the per-group microsecond constants below are this chip's (gfx950, measured: profiles/r5_ubench_gemm_*.txt).  On a part
// with another CU count every tile still computes the same bits - only the CHOICE of tile would be off; the library targets gfx950 alone (Makefile: ARCH).
// Estimated time of a tile shape = rounds of workgroups over the 256 CUs x K groups x the shape's group iteration on a busy CU (us; gemmpipe, w2-like
// launches where every workgroup has a CU to itself: 90.2 / 64, 60.5 / 64, 31.3 / 64 us per group; 96 x 64 between the last two).
GemmTile gemm_q8_ring_tile(int n, int o, int n_tok, bool q4) {
    const int G = n / 128;
    auto cost = [&](int tm, int tn, float per_group) {
        const int wgs = ((o + tm - 1) / tm) * ((n_tok + tn - 1) / tn);
        return (float)((wgs + 255) / 256) * (float)G * per_group;
    };
    const float c256 = cost(256, 128, 1.45f), c128 = cost(128, 128, 0.95f), c64 = cost(64, 64, 0.49f);
    const int wgs64 = ((o + 63) / 64) * ((n_tok + 63) / 64);
    if (q4) {
        // Q4_0 (round 6, measured: profiles/r6_ab_q4_pair_tiles.txt).  The big ring tiles only where they make ONE nearly full turn of workgroups over the 256
        // CUs - Llama-3.2-1B's w1/w3 (256 x 128 at 512 tokens, 128 x 128 at 256), Gemma-2-2B's w1/w3 at 256-384 tokens; everything else - the narrow projections at
        // any length, Gemma's w1/w3 at 512 tokens (288 tiles of 256 x 128: two turns) - on the paired-group column kernel (gemm_q4_pair_kernel), two co-resident
        // workgroups per CU: 64 x 32 tiles while they come to fewer than 512 workgroups, 64 x 64 beyond.  (The Q8_0 cost model above priced Gemma's w2 at 512
        // tokens on 72 tiles of 128 x 128: 115 us; 64 x 64 pairs: fill_kv_cache(512) 10.1 -> 7.6 ms.)
        const int wg256 = ((o + 255) / 256) * ((n_tok + 127) / 128), wg128 = ((o + 127) / 128) * ((n_tok + 127) / 128);
        if (wg256 > 128 && wg256 <= 256) return {256, 128, 8};
        if (wg128 > 128 && wg128 <= 256) return {128, 128, 8};
        const int rt = (o + 63) / 64;
        if (rt * ((n_tok + 31) / 32) < 512) return {64, 32, 4};
        return {64, 64, 4};
    }
    // Launches that 64 x 64 tiles cannot fill the chip with (wo / w2 / qkv of the 2048-wide models up to 256 tokens: 64-192 workgroups on 256 CUs, each
    // bound by its own group iteration): smaller tiles, i.e. more workgroups with shorter iterations - 64 x 32 (0.32 us per group with a CU to itself) and
    // 32 x 32 (two workgroups per CU: 0.24 us up to 256 workgroups, 0.33 up to 512) - profiles/r5_ubench_gemm_narrow.txt: w2 at 256 tokens 29.5 -> 20.5 us,
    // at 128 tokens 27.4 -> 15.5; wo 9.8 -> 7.5 / 9.5 -> 5.9.  The 64 x 64 tile itself runs as 8 waves of 32 x 16 (w2 at 512 tokens 31.2 -> 26.6 us).
    if (wgs64 <= 256) {
        const int w32 = ((o + 31) / 32) * ((n_tok + 31) / 32);
        const float c8 = 0.41f * (float)G, c6432 = cost(64, 32, 0.32f), c32 = (w32 <= 256 ? 0.24f : 0.33f * (float)((w32 + 511) / 512)) * (float)G;
        if (c32 < c6432 && c32 < c8) return {32, 32, 4};
        if (c6432 < c8) return {64, 32, 4};
        return {64, 64, 8};
    }
    // (96 x 64 only where the rows divide and K is short: qkv of the 2048-wide models, 17.5 -> 12.0 us; a ragged 96-row tile or a long K measured slower)
    const float c96 = o % 96 == 0 && n <= 2048 ? cost(96, 64, 0.65f) : 1e30f;
    // (128 x 64, 8 waves of 32 x 32: where it makes ONE round of what 64 x 64 needs two for - wo / w2 of the 3072-wide models at 512 tokens, the image
    //  tower's out_proj / fc2: 0.65-0.73 us per group, profiles/r5_ubench_gemm_tiles_dma.txt)
    const float c12864 = cost(128, 64, 0.69f);
    if (c256 <= c128 && c256 <= c96 && c256 <= c64 && c256 <= c12864) return {256, 128, 8};
    if (c128 <= c96 && c128 <= c64 && c128 <= c12864) return {128, 128, 8};
    if (c12864 < c96 && c12864 < c64) return {128, 64, 8};
    if (c96 <= c64) return {96, 64, 4};
    return {64, 64, 8};
}
// w1/w3 with the h quantiser in the epilogue (EPI_SWIGLU_Q / EPI_GELU_Q): Q8_0, whole 256-row tiles, and a launch big enough for the cost model to ask for
// 256 x 128 or 128 x 128 tiles - the latter runs as 256 x 64 (8 waves of 64 x 32: the same MFMAs and fragment reads per group, 320 rows of DMA instead of 256).
bool gemm_q8_hq_fused(int n, int o, int n_tok, bool q4) {
    if (q4 || o % 256 || n % 256 || n_tok < 48) return false;
    const GemmTile t = gemm_q8_ring_tile(n, o, n_tok, false);
    return t.tm >= 128 && t.tn == 128;
}
template <int EPI>
static hipError_t launch_gemm_q8_ring(const GemmArgs& a, hipStream_t s) {
    const GemmTile t = gemm_q8_ring_tile(a.n, a.o, a.n_tok, a.q4 != 0);
    const int key = t.tm * 1000 + t.tn;
    if constexpr (EPI == EPI_SWIGLU_Q || EPI == EPI_GELU_Q) {
        if (!gemm_q8_hq_fused(a.n, a.o, a.n_tok, a.q4 != 0) || !a.hq || !a.hs) return hipErrorInvalidValue;
        if (key == 256128) return launch_gemm_q8_dma<EPI, 4, 4, 4, 2>(a, s);
        return launch_gemm_q8_dma<EPI, 4, 2, 4, 2>(a, s);
    } else {
        if (a.q4) {                                               // (the text models' epilogues: the image tower's Q4 sections stay on the direct kernel)
            if constexpr (EPI == EPI_STORE || EPI == EPI_RESID || EPI == EPI_QKV || EPI == EPI_SWIGLU || EPI == EPI_GELU) {
                // Q4_0 tiles are COLUMNS of waves (round 6): every wave owns its weight rows against all of the tile's tokens, so a packed row is unpacked by one
                // wave only (with a 2-wide grid of waves the two that shared a row both did it: 62 % more vector instructions per MFMA than Q8_0) -
                // Gemma-2-2B fill_kv_cache(256) 6.31 -> 6.13 ms, w1/w3 66.4 -> 64.1 us, wo / w2 38.8 -> 36.6 (profiles/r6_ab_prefill_fusion.txt); then the
                // small tiles on the paired-group kernel: 5.41 -> 4.93 ms
                switch (key) {
                    case 256128: return launch_gemm_q8_dma<EPI, 2, 8, 8, 1, true>(a, s);       // (as 16 waves on the paired kernel, two slots: spills under its 128-register cap, 4.89 -> 5.24 ms on Gemma-2-2B (256))
                    case 128128: return launch_gemm_q4_pair<EPI, 8, 8, 3>(a, s);               // 8 waves, three pairs: Llama-3.2-1B Q4_0 (256) 2.24 -> 2.17 ms, Gemma-2-2B (128) 3.85 -> 3.79
                    case 64032: return launch_gemm_q4_pair<EPI, 2, 4, 4>(a, s);       // small tiles: a ring slot = a PAIR of groups, whole cache lines of packed weights
                    default: return launch_gemm_q4_pair<EPI, 4, 4, 3>(a, s);         // 64 x 64: three slots, so that two workgroups share a CU
                }
            } else return hipErrorNotSupported;
        }
        switch (key) {
            case 256128: return launch_gemm_q8_dma<EPI, 4, 4, 4, 2>(a, s);
            case 128128: return launch_gemm_q8_dma<EPI, 2, 4, 4, 2>(a, s);
            case 128064: return launch_gemm_q8_dma<EPI, 2, 2, 4, 2>(a, s);
            case 96064: return launch_gemm_q8_dma<EPI, 3, 2, 2, 2>(a, s);
            case 64032: return launch_gemm_q8_dma<EPI, 2, 1, 2, 2>(a, s);
            case 32032: return launch_gemm_q8_dma<EPI, 1, 1, 2, 2>(a, s);
            default: return launch_gemm_q8_dma<EPI, 2, 1, 2, 4>(a, s);
        }
    }
}
template <int EPI>
static hipError_t launch_gemm_q8_epi(const GemmArgs& a, hipStream_t s) {
    const int rt = (a.o + 31) / 32, tt = (a.n_tok + 63) / 64;
    const size_t sc1 = (size_t)(a.n / 128) * (32 + 64) * sizeof(float);       // group scales of one wave's 32 rows and 64 tokens
    if (a.q4) {                                                   // packed-nibble weights: the ring kernel from 48 tokens on (text models), else the direct kernel unpacks its fragments
        if (a.n_tok >= 48) { const hipError_t e = launch_gemm_q8_ring<EPI>(a, s); if (e != hipErrorNotSupported) return e; }
        if (sc1 > 150 * 1024) return hipErrorInvalidValue;
        if ((rt / 4) * tt >= 256 && 4 * sc1 <= 150 * 1024) { allow_big_lds(reinterpret_cast<const void*>(gemm_q8_kernel<EPI, 2, 4, 4, true>)); hipLaunchKernelGGL((gemm_q8_kernel<EPI, 2, 4, 4, true>), dim3((rt + 3) / 4, tt), dim3(256), 4 * sc1, s, a); }
        else { allow_big_lds(reinterpret_cast<const void*>(gemm_q8_kernel<EPI, 2, 4, 1, true>)); hipLaunchKernelGGL((gemm_q8_kernel<EPI, 2, 4, 1, true>), dim3(rt, tt), dim3(64), sc1, s, a); }
        return hipGetLastError();
    }
    // Q8_0 at 48 tokens or more: the LDS-DMA ring kernel, its tile chosen by shape (below 48 tokens a token tile is mostly padding: the kernels below)
    if (a.n_tok >= 48) return launch_gemm_q8_ring<EPI>(a, s);
    if (sc1 > 150 * 1024) return hipErrorInvalidValue;
    if ((rt / 4) * tt >= 256 && 4 * sc1 <= 150 * 1024) { allow_big_lds(reinterpret_cast<const void*>(gemm_q8_kernel<EPI, 2, 4, 4>)); hipLaunchKernelGGL((gemm_q8_kernel<EPI, 2, 4, 4>), dim3((rt + 3) / 4, tt), dim3(256), 4 * sc1, s, a); return hipGetLastError(); }
    // few tiles, long K: four waves per tile, the group sums handed round in order (gemm_q8_ring_kernel)
    if ((a.n / 128) % 4 == 0 && a.n_tok >= 17 && rt * tt <= 320) {
        const size_t smem = 2 * 4 * 8 * 64 * 16 + sc1;                                // two rounds of the four waves' products + their group scales
        allow_big_lds(reinterpret_cast<const void*>(gemm_q8_ring_kernel<EPI>));
        hipLaunchKernelGGL((gemm_q8_ring_kernel<EPI>), dim3(rt, tt), dim3(256), smem, s, a);
        return hipGetLastError();
    }
    // (smaller wave tiles - 16 x 32, 32 x 32, 16 x 64 - put more waves on a CU but move more bytes per MAC: measured slower)
    allow_big_lds(reinterpret_cast<const void*>(gemm_q8_kernel<EPI, 2, 4, 1>));
    hipLaunchKernelGGL((gemm_q8_kernel<EPI, 2, 4, 1>), dim3(rt, tt), dim3(64), sc1, s, a);
    return hipGetLastError();
}
// ------------------------------------------------------------------------------------------------
// Skinny GEMM: 1 .. 16 tokens (GemmArgs::skinny; a drafted run to verify, a chat turn, a prompt tail).  The token axis is ONE 16-wide MFMA tile, so a pass
// is a weight stream, like a decode step's GEMVs: every weight byte is read from HBM once (wide non-temporal loads) whatever n_tok is, and what has to be
// found is bytes in flight, not MFMAs.  A workgroup of NW waves owns 16 MT weight rows; wave w takes the groups g = w (mod NW) - its loads, MFMAs and the two
// multiplies per element need no order - keeps D groups of fragments in flight in registers and parks its products ((isum as f32) * ws) * xs in LDS, [g][tile][lane].
// Only the ADD is ordered (the reference adds a row's group products in ascending group order): after the one barrier of the kernel wave m adds the products
// of row tile m, g = 0 .. G - 1, and runs the epilogue.  Same operations in the same order per element as gemm_q8_kernel: bit-identical.
// Activations: the n_tok int8 rows are MFMA fragments straight from global memory (L2: they are a few KB .. 144 KB and every workgroup reads them), one pair
// of fragments per group shared by the MT row tiles of a wave; tokens past the batch are a duplicate of the last one and never stored.  The group scales of
// a wave's own groups are staged in LDS by that wave before its first group ([i][row] / [i][token], as gemm_q8_kernel: no loop-carried loaded scalars).
// Scale layout: ROW-MAJOR only (ws [o][n/128], xs [n_tok][n/128]; ws_ld / xs_ld must be 0 - the launcher refuses others): what a pass below 48 tokens uses.
// ------------------------------------------------------------------------------------------------
#ifndef LMRS_SKINNY_DEPTH
#define LMRS_SKINNY_DEPTH 2                                      // groups of fragments a wave keeps in flight (measured: 4 is slower, profiles/ab_skinny_tile.txt; A/B builds: make V=.. EXTRA=-DLMRS_SKINNY_DEPTH=4)
#endif
#ifndef LMRS_SKINNY_WIDE_ROWS
#define LMRS_SKINNY_WIDE_ROWS 8192                               // launches of at least this many rows take the 32-row tiles
#endif
template <int EPI, int MT, int NW, bool Q4 = false>
__global__ __launch_bounds__(64 * NW) void gemm_skinny_kernel(const GemmArgs a) {
    constexpr int D = LMRS_SKINNY_DEPTH;
    constexpr int NR = 16 * MT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, kb = lane >> 4;
    const int K = a.n, G = K / 128, GW = (G + NW - 1) / NW;      // GW: groups per wave, rounded up (a wave's surplus turns re-load its last group, their products go to the dump slot G)
    const int WB = Q4 ? K / 2 : K;
    const int r0 = blockIdx.x * NR;
    f32x4m* P = reinterpret_cast<f32x4m*>(smem_raw);             // [G + 1][MT][64 lanes] products
    float* wsl = reinterpret_cast<float*>(smem_raw + (size_t)(G + 1) * MT * 1024) + (size_t)wave * GW * (NR + 16);   // this wave's groups: [GW][NR]
    float* xsl = wsl + (size_t)GW * NR;                                                                              //                     [GW][16]
    const int8_t* wrow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int r = r0 + m * 16; r = r < a.o ? r : a.o - 16;         // a ragged last tile re-does the previous one (o is a multiple of 16)
        wrow[m] = static_cast<const int8_t*>(a.wq) + (size_t)(r + lr) * WB + kb * (Q4 ? 8 : 16);
    }
    const int8_t* xrow;
    { const int t = lr < a.n_tok ? lr : a.n_tok - 1; xrow = a.xq + (size_t)t * K + kb * 16; }
    typedef int i32x2m __attribute__((ext_vector_type(2)));
    using WFrag = std::conditional_t<Q4, i32x2m, i32x4m>;        // Q4: the packed bytes stay packed until the MFMA (half the registers in flight)
    struct Frag { WFrag w0[MT], w1[MT]; i32x4m x0, x1; };
    auto group_of = [&](int i) __attribute__((always_inline)) { const int g = i * NW + wave; return g < G ? g : G - 1; };     // (clamped: always a valid address)
    auto load = [&](Frag& f, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f.w0[m] = __builtin_nontemporal_load(reinterpret_cast<const WFrag*>(wrow[m] + (size_t)g * (Q4 ? 64 : 128)));
            f.w1[m] = __builtin_nontemporal_load(reinterpret_cast<const WFrag*>(wrow[m] + (size_t)g * (Q4 ? 64 : 128) + (Q4 ? 32 : 64)));
        }
        f.x0 = *reinterpret_cast<const i32x4m*>(xrow + (size_t)g * 128);
        f.x1 = *reinterpret_cast<const i32x4m*>(xrow + (size_t)g * 128 + 64);
    };
    Frag f[D];
#pragma unroll
    for (int k = 0; k < D; ++k) load(f[k], group_of(k));         // the weight stream starts before the scales are staged
    {   // group scales of this wave's groups (turn i -> group_of(i)): lane -> (row, turn phase) / (token, turn phase)
        int r = r0 + (lane % NR); r = r < a.o ? r : a.o - 1;
        const float* wsp = a.ws + (size_t)r * G;
        for (int i = lane / NR; i < GW; i += 64 / NR) wsl[i * NR + (lane % NR)] = wsp[group_of(i)];
        const int t = lr < a.n_tok ? lr : a.n_tok - 1;
        const float* xsp = a.xs + (size_t)t * G;
        for (int i = kb; i < GW; i += 4) xsl[i * 16 + lr] = xsp[group_of(i)];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                             // (each wave reads only the scales it wrote)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto use = [&](const Frag& fr, int i) __attribute__((always_inline)) {
        const int ic = i < GW ? i : GW - 1, g = i * NW + wave, slot = (i < GW && g < G) ? g : G;
        const float xsv = xsl[ic * 16 + lr];
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const f32x4m wsv = *reinterpret_cast<const f32x4m*>(wsl + ic * NR + m * 16 + kb * 4);     // the 4 weight rows this lane holds
            i32x4m w0, w1, c = {0, 0, 0, 0};
            if constexpr (Q4) { w0 = q4_fragment(fr.w0[m].x, fr.w0[m].y); w1 = q4_fragment(fr.w1[m].x, fr.w1[m].y); }
            else { w0 = fr.w0[m]; w1 = fr.w1[m]; }
            c = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, fr.x0, c, 0, 0, 0);                           // D[row = weight row][col = token]
            c = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, fr.x1, c, 0, 0, 0);
            f32x4m p;
#pragma unroll
            for (int e = 0; e < 4; ++e) { float q = (float)c[e] * wsv[e]; p[e] = q * xsv; }             // ((ival as f32) * w.s[..]) * x.s[..]
            P[((size_t)slot * MT + m) * 64 + lane] = p;
        }
    };
    for (int i = 0; i < GW; i += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            use(f[k], i + k);
            { const int in = i + k + D; load(f[k], group_of(in < GW ? in : GW - 1)); }      // unconditional (the tail re-loads the wave's last group: no load under a branch)
        }
    }
    __syncthreads();
    // ---- the ordered sum: wave m < MT adds the products of row tile m in ascending group order, then the epilogue of gemm_q8_kernel
    if (wave < MT) {
        const int m = wave;
        f32x4m acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int g = 0; g < G; ++g) {
            const f32x4m v = P[((size_t)g * MT + m) * 64 + lane];
            acc[0] = acc[0] + v[0]; acc[1] = acc[1] + v[1]; acc[2] = acc[2] + v[2]; acc[3] = acc[3] + v[3];
        }
        if (r0 + m * 16 < a.o && lr < a.n_tok) gemm_epilogue<EPI>(a, r0 + m * 16 + kb * 4, lr, acc[0], acc[1], acc[2], acc[3]);
    }
}
static size_t gemm_skinny_lds(int n, int mt, int nw) {
    const int G = n / 128, GW = (G + nw - 1) / nw;
    return (size_t)(G + 1) * mt * 1024 + (size_t)nw * GW * (16 * mt + 16) * sizeof(float);
}
// The tile by shape: launches of few rows (wo, w2, qkv: a few hundred 16-row tiles) put 8 waves on every tile, so that the launch has a few thousand waves'
// loads in flight; the wide ones (w1/w3, the classifier) take 32-row tiles of 4 waves, whose two row tiles share the activation fragments.
template <int EPI, bool Q4>
static hipError_t launch_gemm_skinny(const GemmArgs& a, hipStream_t s) {
    if (a.ws_ld || a.xs_ld || a.n_tok > 16) return hipErrorInvalidValue;
    const size_t wide = gemm_skinny_lds(a.n, 2, 4), narrow = gemm_skinny_lds(a.n, 1, 8);
    if (a.o >= LMRS_SKINNY_WIDE_ROWS && wide <= 64 * 1024) {
        hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 2, 4, Q4>), dim3((a.o + 31) / 32), dim3(256), wide, s, a);
        return hipGetLastError();
    }
    if (narrow > 150 * 1024) return hipErrorInvalidValue;
    allow_big_lds(reinterpret_cast<const void*>(gemm_skinny_kernel<EPI, 1, 8, Q4>));
    hipLaunchKernelGGL((gemm_skinny_kernel<EPI, 1, 8, Q4>), dim3(a.o / 16), dim3(512), narrow, s, a);
    return hipGetLastError();
}
static hipError_t launch_gemm_skinny_epi(const GemmArgs& a, int epi, hipStream_t s) {
#define SK(E_) case E_: return a.q4 ? launch_gemm_skinny<E_, true>(a, s) : launch_gemm_skinny<E_, false>(a, s)
    switch (epi) {
        SK(EPI_STORE); SK(EPI_RESID); SK(EPI_QKV); SK(EPI_SWIGLU); SK(EPI_GELU);
        default: return hipErrorInvalidValue;                     // (the text pass's epilogues only; the quantising forms are not needed below 128-token tiles)
    }
#undef SK
}
// ------------------------------------------------------------------------------------------------
// Stream GEMM: 17 .. 47 tokens of a batch pass (GemmArgs::skinny with more than one token tile; the kernel itself serves 1 .. 64, the callers' limit is measured).  The skinny kernel's
// weight stream - every weight byte read from HBM once, wide non-temporal loads, Q4_0 rows packed until the MFMA - against NT = 2 .. 4 token tiles: a weight
// fragment in registers meets all NT activation tiles before it is dropped.  The skinny kernel parks EVERY group's products in LDS ((G + 1) x MT KiB per
// token tile: 260 KiB for K = 8192 at four tiles), so here K goes in ROUNDS of NW groups, one per wave: round t's products ((isum as f32) * ws) * xs go to
// slab t & 1 ([wave][token tile][row tile][lane]); behind the round's barrier the adder waves - one per output tile, tile q on wave q mod NW - add the
// round's products to an accumulator they keep in registers, in ascending group order, while every wave forms round t + 1's products in the other slab.
// One barrier per round: slab t & 1 is written again in round t + 2, behind the barrier of round t + 1, which the adds of round t precede.
// Same operations in the same order per element as gemm_skinny_kernel / gemm_q8_kernel: bit-identical.  Tokens past n_tok duplicate the last token and are
// never stored; a ragged last row tile re-does the previous one.  Scales: ROW-MAJOR only, staged per wave as the skinny kernel stages them.
// One group of fragments in flight per wave (LMRS_STREAM_DEPTH): the registers a second one takes cost more resident waves than it hides latency.
// LDS: 2 NW NT MT KiB of slabs (64 KiB at four token tiles) + the scales (23 KiB for K = 9216).
// ------------------------------------------------------------------------------------------------
#ifndef LMRS_STREAM_DEPTH
#define LMRS_STREAM_DEPTH 1                                      // groups of fragments a wave keeps in flight (measured: 2 is slower at every row count, profiles/ab_stream_tile.txt; A/B builds: make V=.. EXTRA=-DLMRS_STREAM_DEPTH=2)
#endif
#ifndef LMRS_STREAM_WIDE_ROWS
#define LMRS_STREAM_WIDE_ROWS 8192                               // launches of at least this many rows take the 32-row tiles of 4 waves (as LMRS_SKINNY_WIDE_ROWS)
#endif
template <int EPI, int NT, int MT, int NW, bool Q4 = false>
__global__ __launch_bounds__(64 * NW) void gemm_stream_kernel(const GemmArgs a) {
    constexpr int D = LMRS_STREAM_DEPTH;
    constexpr int NR = 16 * MT, TK = 16 * NT, NQ = NT * MT, NA = (NQ + NW - 1) / NW;      // NQ output tiles, NA of them per adder wave
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, kb = lane >> 4;
    const int K = a.n, G = K / 128, GW = (G + NW - 1) / NW;      // GW rounds; a wave without a group in the last round re-does group G - 1, nobody adds its products
    const int WB = Q4 ? K / 2 : K;
    const int r0 = blockIdx.x * NR;
    f32x4m* P = reinterpret_cast<f32x4m*>(smem_raw);             // [2][NW][NQ][64 lanes] products
    float* wsl = reinterpret_cast<float*>(smem_raw + (size_t)2 * NW * NQ * 1024) + (size_t)wave * GW * (NR + TK);     // this wave's groups: [GW][NR]
    float* xsl = wsl + (size_t)GW * NR;                                                                               //                     [GW][TK]
    const int8_t* wrow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        int r = r0 + m * 16; r = r < a.o ? r : a.o - 16;         // a ragged last tile re-does the previous one (o is a multiple of 16)
        wrow[m] = static_cast<const int8_t*>(a.wq) + (size_t)(r + lr) * WB + kb * (Q4 ? 8 : 16);
    }
    const int8_t* xrow[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { int t = j * 16 + lr; t = t < a.n_tok ? t : a.n_tok - 1; xrow[j] = a.xq + (size_t)t * K + kb * 16; }
    typedef int i32x2m __attribute__((ext_vector_type(2)));
    using WFrag = std::conditional_t<Q4, i32x2m, i32x4m>;
    struct Frag { WFrag w0[MT], w1[MT]; i32x4m x0[NT], x1[NT]; };
    auto group_of = [&](int i) __attribute__((always_inline)) { const int g = i * NW + wave; return g < G ? g : G - 1; };     // (clamped: always a valid address)
    auto load = [&](Frag& f, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            f.w0[m] = __builtin_nontemporal_load(reinterpret_cast<const WFrag*>(wrow[m] + (size_t)g * (Q4 ? 64 : 128)));
            f.w1[m] = __builtin_nontemporal_load(reinterpret_cast<const WFrag*>(wrow[m] + (size_t)g * (Q4 ? 64 : 128) + (Q4 ? 32 : 64)));
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            f.x0[j] = *reinterpret_cast<const i32x4m*>(xrow[j] + (size_t)g * 128);
            f.x1[j] = *reinterpret_cast<const i32x4m*>(xrow[j] + (size_t)g * 128 + 64);
        }
    };
    Frag f[D];
#pragma unroll
    for (int k = 0; k < D; ++k) load(f[k], group_of(k < GW ? k : GW - 1));      // the weight stream starts before the scales are staged
    for (int e = lane; e < GW * NR; e += 64) {                  // group scales of this wave's groups (round i -> group_of(i))
        const int i = e / NR; int r = r0 + (e - i * NR); r = r < a.o ? r : a.o - 1;
        wsl[e] = a.ws[(size_t)r * G + group_of(i)];
    }
    for (int e = lane; e < GW * TK; e += 64) {
        const int i = e / TK; int t = e - i * TK; t = t < a.n_tok ? t : a.n_tok - 1;
        xsl[e] = a.xs[(size_t)t * G + group_of(i)];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();                             // (each wave reads only the scales it wrote)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto use = [&](const Frag& fr, int i) __attribute__((always_inline)) {
        f32x4m* slab = P + ((size_t)(i & 1) * NW + wave) * NQ * 64;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const f32x4m wsv = *reinterpret_cast<const f32x4m*>(wsl + i * NR + m * 16 + kb * 4);      // the 4 weight rows this lane holds
            i32x4m w0, w1;
            if constexpr (Q4) { w0 = q4_fragment(fr.w0[m].x, fr.w0[m].y); w1 = q4_fragment(fr.w1[m].x, fr.w1[m].y); }
            else { w0 = fr.w0[m]; w1 = fr.w1[m]; }
#pragma unroll
            for (int j = 0; j < NT; ++j) {                       // the fragment against every token tile
                const float xsv = xsl[i * TK + j * 16 + lr];
                i32x4m c = {0, 0, 0, 0};
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, fr.x0[j], c, 0, 0, 0);                    // D[row = weight row][col = token]
                c = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, fr.x1[j], c, 0, 0, 0);
                f32x4m p;
#pragma unroll
                for (int e = 0; e < 4; ++e) { float q = (float)c[e] * wsv[e]; p[e] = q * xsv; }         // ((ival as f32) * w.s[..]) * x.s[..]
                slab[(j * MT + m) * 64 + lane] = p;
            }
        }
    };
    f32x4m acc[NA];
#pragma unroll
    for (int u = 0; u < NA; ++u) acc[u] = f32x4m{0.f, 0.f, 0.f, 0.f};
    // the ordered sum of round i: its groups i NW .. in ascending order onto the tiles this wave owns
    auto add = [&](int i) __attribute__((always_inline)) {
        const int cnt = G - i * NW < NW ? G - i * NW : NW;
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int q = wave + u * NW;
            if (q < NQ) {
                const f32x4m* src = P + (size_t)(i & 1) * NW * NQ * 64 + q * 64 + lane;
                for (int w = 0; w < cnt; ++w) {
                    const f32x4m v = src[(size_t)w * NQ * 64];
                    acc[u][0] = acc[u][0] + v[0]; acc[u][1] = acc[u][1] + v[1]; acc[u][2] = acc[u][2] + v[2]; acc[u][3] = acc[u][3] + v[3];
                }
            }
        }
    };
    for (int i = 0; i < GW; i += D) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
            if (i + k < GW) {                                    // (uniform over the workgroup: every wave meets the same barriers)
                use(f[k], i + k);
                { const int in = i + k + D; load(f[k], group_of(in < GW ? in : GW - 1)); }
                if (i + k > 0) add(i + k - 1);                   // round i + k - 1's adds under this round's loads
                __syncthreads();
            }
        }
    }
    add(GW - 1);
#pragma unroll
    for (int u = 0; u < NA; ++u) {
        const int q = wave + u * NW, j = q / MT, m = q - j * MT, t = j * 16 + lr;
        if (q < NQ && r0 + m * 16 < a.o && t < a.n_tok) gemm_epilogue<EPI>(a, r0 + m * 16 + kb * 4, t, acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
    }
}
constexpr int kStreamTokens = 64;                                // four token tiles
static size_t gemm_stream_lds(int n, int nt, int mt, int nw) {
    const int G = n / 128, GW = (G + nw - 1) / nw;
    return (size_t)2 * nw * nt * mt * 1024 + (size_t)nw * GW * (16 * mt + 16 * nt) * sizeof(float);
}
// The tile by shape, as the skinny kernel's: few rows (wo, w2, qkv) on 16-row tiles of 8 waves, the wide launches (w1/w3, the classifier) on 32-row tiles of
// 4 waves, whose two row tiles share the activation fragments (half the L2 traffic per weight byte).
template <int EPI, int NT, bool Q4>
static hipError_t launch_gemm_stream_nt(const GemmArgs& a, hipStream_t s) {
    const size_t wide = gemm_stream_lds(a.n, NT, 2, 4), narrow = gemm_stream_lds(a.n, NT, 1, 8);
    if (wide > 150 * 1024 || narrow > 150 * 1024) return hipErrorInvalidValue;
    if (a.o >= LMRS_STREAM_WIDE_ROWS) {
        allow_big_lds(reinterpret_cast<const void*>(gemm_stream_kernel<EPI, NT, 2, 4, Q4>));
        hipLaunchKernelGGL((gemm_stream_kernel<EPI, NT, 2, 4, Q4>), dim3((a.o + 31) / 32), dim3(256), wide, s, a);
        return hipGetLastError();
    }
    allow_big_lds(reinterpret_cast<const void*>(gemm_stream_kernel<EPI, NT, 1, 8, Q4>));
    hipLaunchKernelGGL((gemm_stream_kernel<EPI, NT, 1, 8, Q4>), dim3(a.o / 16), dim3(512), narrow, s, a);
    return hipGetLastError();
}
template <int EPI, bool Q4>
static hipError_t launch_gemm_stream(const GemmArgs& a, hipStream_t s) {
    if (a.ws_ld || a.xs_ld || a.n_tok > kStreamTokens) return hipErrorInvalidValue;
    if (a.n_tok <= 32) return launch_gemm_stream_nt<EPI, 2, Q4>(a, s);
    if (a.n_tok <= 48) return launch_gemm_stream_nt<EPI, 3, Q4>(a, s);
    return launch_gemm_stream_nt<EPI, 4, Q4>(a, s);
}
static hipError_t launch_gemm_stream_epi(const GemmArgs& a, int epi, hipStream_t s) {
#define ST(E_) case E_: return a.q4 ? launch_gemm_stream<E_, true>(a, s) : launch_gemm_stream<E_, false>(a, s)
    switch (epi) {
        ST(EPI_STORE); ST(EPI_RESID); ST(EPI_QKV); ST(EPI_SWIGLU); ST(EPI_GELU);
        default: return hipErrorInvalidValue;                     // (the text pass's epilogues, as launch_gemm_skinny_epi)
    }
#undef ST
}
// lmrs_debug_gemm_wide: the stream kernel at any n_tok it serves (the dispatch below sends it 17 .. 64, its callers ask up to 47)
hipError_t launch_gemm_stream_store(const GemmArgs& a, hipStream_t s) {
    if (a.n % 256 || a.o % 16 || a.n_tok <= 0) return hipErrorInvalidValue;
    return launch_gemm_stream_epi(a, EPI_STORE, s);
}

hipError_t launch_gemm_q8(const GemmArgs& a, int epi, hipStream_t s) {
    if (a.n % 256 || a.o % 16 || a.n_tok <= 0) return hipErrorInvalidValue;
    if (a.skinny && a.n_tok <= 16) return launch_gemm_skinny_epi(a, epi, s);
    if (a.skinny && a.n_tok <= kStreamTokens) return launch_gemm_stream_epi(a, epi, s);
    switch (epi) {
        case EPI_STORE: return launch_gemm_q8_epi<EPI_STORE>(a, s);
        case EPI_RESID: return launch_gemm_q8_epi<EPI_RESID>(a, s);
        case EPI_QKV: return launch_gemm_q8_epi<EPI_QKV>(a, s);
        case EPI_SWIGLU: return launch_gemm_q8_epi<EPI_SWIGLU>(a, s);
        case EPI_GELU: return launch_gemm_q8_epi<EPI_GELU>(a, s);
        case EPI_VQKV: return launch_gemm_q8_epi<EPI_VQKV>(a, s);
        case EPI_BIAS_RESID: return launch_gemm_q8_epi<EPI_BIAS_RESID>(a, s);
        case EPI_BIAS_QGELU: return launch_gemm_q8_epi<EPI_BIAS_QGELU>(a, s);
        case EPI_BIAS_GELU: return launch_gemm_q8_epi<EPI_BIAS_GELU>(a, s);
        case EPI_BIAS: return launch_gemm_q8_epi<EPI_BIAS>(a, s);
        case EPI_SWIGLU_Q: return launch_gemm_q8_ring<EPI_SWIGLU_Q>(a, s);
        case EPI_GELU_Q: return launch_gemm_q8_ring<EPI_GELU_Q>(a, s);
        default: return hipErrorInvalidValue;
    }
}

// ------------------------------------------------------------------------------------------------
// Per-token prologue for a batch: ([x += rmsnorm(delta)] [rmsnorm]) quantize of every row, one workgroup per token, the
// static-shape functions of lmrs_stage.h (same arithmetic as the GEMV prologues).  x [n_tok][N] f32 -> xq [n_tok][N] int8,
// xs [n_tok][N/128].  MODE 0: quantize; 1: rmsnorm, quantize; 2 (Gemma): x += rmsnorm(delta, add_w) stored back, then as 1.
// Q4: the reference's Q4_0 activation quantiser; the values (q - 8) are stored as int8, de-interleaved within every 8
// elements as [e0 e2 e4 e6 | e1 e3 e5 e7] - the order gemm_q8_kernel's unpacked weight fragments have.
// ------------------------------------------------------------------------------------------------
template <int N, int NTH, int MODE, bool Q4>
__global__ __launch_bounds__(NTH) void rows_prologue_kernel(float* x, const float* rms_w, const float* delta, const float* add_w, float eps, int add_unit,
                                                            int8_t* xq_out, float* xs_out, int xs_ld) {
    __shared__ __attribute__((aligned(16))) int8_t xq[N];
    __shared__ float xs[N / 128];
    __shared__ __attribute__((aligned(16))) float scratch[MODE ? rms_scratch_floats(N) : 4];
    using V = VecGeom<N, NTH>;
    const size_t tok = blockIdx.x;
    float4 v[V::NP], nw[V::NP];
    vec_load<N, false, NTH>(v, x + tok * N);
    if constexpr (MODE == 2) {
        float4 dl[V::NP], aw[V::NP];
        vec_load<N, false, NTH>(dl, delta + tok * N); vec_load<N, false, NTH>(aw, add_w);
        vec_rmsnorm<N, NTH>(dl, aw, eps, add_unit, scratch);
#pragma unroll
        for (int i = 0; i < V::NP; ++i) {
            v[i].x = v[i].x + dl[i].x; v[i].y = v[i].y + dl[i].y; v[i].z = v[i].z + dl[i].z; v[i].w = v[i].w + dl[i].w;
            const int e = V::elem(i, (int)threadIdx.x);
            if (V::FULL || i < V::NP - 1 || e < N) *reinterpret_cast<float4*>(x + tok * N + e) = v[i];
        }
    }
    if constexpr (MODE >= 1) { vec_load<N, false, NTH>(nw, rms_w); vec_rmsnorm<N, NTH>(v, nw, eps, add_unit, scratch); }
    if constexpr (!Q4) {
        vec_quantize_q8<N, NTH>(v, xq, xs);
        lds_barrier();
        for (int e = threadIdx.x * 16; e < N; e += NTH * 16) *reinterpret_cast<int4*>(xq_out + tok * N + e) = *reinterpret_cast<const int4*>(xq + e);
    } else {
        vec_quantize_q4<N, NTH>(v, xq, xs);                      // packed nibbles ^ 8 in the first N / 2 bytes
        lds_barrier();
        for (int e = threadIdx.x * 8; e < N; e += NTH * 8) {    // 8 elements = one packed dword -> 8 signed bytes, evens then odds
            const unsigned w = *reinterpret_cast<const unsigned*>(xq + (e >> 1)) ^ 0x88888888u;   // back to the plain nibbles
            int2 o; o.x = nib_signed(w); o.y = nib_signed(w >> 4);
            *reinterpret_cast<int2*>(xq_out + tok * N + e) = o;
        }
    }
    for (int g = threadIdx.x; g < N / 128; g += NTH) { if (xs_ld) xs_out[(size_t)g * xs_ld + tok] = xs[g]; else xs_out[tok * (N / 128) + g] = xs[g]; }
}

bool rows_prologue_supported(int n) { return n == 2048 || n == 3072 || n == 8192 || n == 2304 || n == 9216 || n == 1024 || n == 4096; }

// mode: 0 quantize, 1 rmsnorm + quantize, 2 x += rmsnorm(delta, add_w) then rmsnorm + quantize
hipError_t launch_rows_prologue(float* x, const float* rms_w, const float* delta, const float* add_w, float eps, int add_unit, int mode, int q4,
                                int n, int n_tok, int8_t* xq, float* xs, hipStream_t s, int xs_ld) {
#define RPK(N_, NT_, M_, Q_) hipLaunchKernelGGL((rows_prologue_kernel<N_, NT_, M_, Q_>), dim3(n_tok), dim3(NT_), 0, s, x, rms_w, delta, add_w, eps, add_unit, xq, xs, xs_ld)
#define RP(N_, NT_)                                                                                       \
    if (n == N_) {                                                                                        \
        if (mode == 0) { if (q4) RPK(N_, NT_, 0, true); else RPK(N_, NT_, 0, false); }                    \
        else if (mode == 1) { if (q4) RPK(N_, NT_, 1, true); else RPK(N_, NT_, 1, false); }               \
        else { if (q4) RPK(N_, NT_, 2, true); else RPK(N_, NT_, 2, false); }                              \
        return hipGetLastError();                                                                         \
    }
    // (4096, 8192 and 9216 are hidden sizes, quantised only, and model widths of Llama / Phi geometries, normed too; mode 2 is Gemma-2's, whose width is 2304)
#define RP1(N_, NT_)                                                                                      \
    if (n == N_) {                                                                                        \
        if (mode == 0) { if (q4) RPK(N_, NT_, 0, true); else RPK(N_, NT_, 0, false); }                    \
        else if (mode == 1) { if (q4) RPK(N_, NT_, 1, true); else RPK(N_, NT_, 1, false); }               \
        else return hipErrorInvalidValue;                                                                 \
        return hipGetLastError();                                                                         \
    }
    RP(2048, 256) RP(3072, 256) RP1(8192, 512) RP(2304, 256) RP1(9216, 512) RP(1024, 256) RP1(4096, 512)
#undef RP1
#undef RP
#undef RPK
    return hipErrorInvalidValue;
}

// Gemma, after the last layer of a batch: x += rmsnorm(delta, w) per token (transformer.rs:643-650)
template <int N, int NTH>
__global__ __launch_bounds__(NTH) void rows_addnorm_kernel(float* x, const float* delta, const float* w, float eps) {
    __shared__ __attribute__((aligned(16))) float scratch[rms_scratch_floats(N)];
    using V = VecGeom<N, NTH>;
    const size_t tok = blockIdx.x;
    float4 v[V::NP], dl[V::NP], aw[V::NP];
    vec_load<N, false, NTH>(v, x + tok * N); vec_load<N, false, NTH>(dl, delta + tok * N); vec_load<N, false, NTH>(aw, w);
    vec_rmsnorm<N, NTH>(dl, aw, eps, 1, scratch);
#pragma unroll
    for (int i = 0; i < V::NP; ++i) {
        v[i].x = v[i].x + dl[i].x; v[i].y = v[i].y + dl[i].y; v[i].z = v[i].z + dl[i].z; v[i].w = v[i].w + dl[i].w;
        const int e = V::elem(i, (int)threadIdx.x);
        if (V::FULL || i < V::NP - 1 || e < N) *reinterpret_cast<float4*>(x + tok * N + e) = v[i];
    }
}
hipError_t launch_rows_addnorm(float* x, const float* delta, const float* w, float eps, int n, int n_tok, hipStream_t s) {
    if (n != 2304) return hipErrorInvalidValue;
    hipLaunchKernelGGL((rows_addnorm_kernel<2304, 256>), dim3(n_tok), dim3(256), 0, s, x, delta, w, eps);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// RoPE for a batch (transformer.rs:443-495): q rotated in place, k rotated into the (blocked) K cache at pos0 + t.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rope_rows_kernel(float* q, const float* k_raw, float* k_cache, const float* rope, int n_heads, int n_kv_heads,
                                                         int hs, int seq_len, int layer, int pos0) {
    const int t = blockIdx.x, pos = pos0 + t, half = hs / 2;
    const int att = n_heads * hs, kv = n_kv_heads * hs;
    for (int i = threadIdx.x; i < (n_heads + n_kv_heads) * half; i += blockDim.x) {
        const int hh = i / half, j = i - hh * half;
        const float2 cs = *reinterpret_cast<const float2*>(rope + ((size_t)pos * half + j) * 2);
        const float fcr = cs.x, fci = cs.y;
        if (hh < n_heads) {
            float* p = q + (size_t)t * att + hh * hs;
            const float v0 = p[j], v1 = p[j + half];
            const float a0 = v0 * fcr, a1 = v1 * fci, b0 = v0 * fci, b1 = v1 * fcr;
            p[j] = a0 - a1; p[j + half] = b0 + b1;
        } else {
            const int kvh = hh - n_heads;
            const float* p = k_raw + (size_t)t * kv + kvh * hs;
            const float v0 = p[j], v1 = p[j + half];
            const float a0 = v0 * fcr, a1 = v1 * fci, b0 = v0 * fci, b1 = v1 * fcr;
            float* kT = k_cache + ((size_t)layer * n_kv_heads + kvh) * hs * (size_t)seq_len;
            kT[(((size_t)(j >> 2) * seq_len + pos) << 2) + (j & 3)] = a0 - a1;
            kT[(((size_t)((j + half) >> 2) * seq_len + pos) << 2) + ((j + half) & 3)] = b0 + b1;
        }
    }
}

hipError_t launch_rope_rows(float* q, const float* k_raw, float* k_cache, const float* rope, int n_heads, int n_kv_heads, int hs, int seq_len,
                            int layer, int pos0, int n_tok, hipStream_t s) {
    hipLaunchKernelGGL(rope_rows_kernel, dim3(n_tok), dim3(256), 0, s, q, k_raw, k_cache, rope, n_heads, n_kv_heads, hs, seq_len, layer, pos0);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Attention for a batch: grid (heads, tokens); token i sits at position pos0 + i and sees keys 0 .. pos0 + i
// (transformer.rs:501-544 inside the sl loop).  q is already rotated and every key of the batch already in the cache.
// ------------------------------------------------------------------------------------------------
template <int HS, bool GEMMA>
__global__ __launch_bounds__(kBlock) void attention_rows_kernel(const AttnArgs a0, int pos0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AttnArgs a = a0;
    const int h = blockIdx.x, tok = gridDim.y - 1 - blockIdx.y, att = a.n_heads * HS;   // the last tokens see the most keys: dispatched first (no long tail)
    a.q = a0.q + (size_t)tok * att; a.out = a0.out + (size_t)tok * att; a.dbg = nullptr;
    const uint64_t etab = exp2f_tab_lane();
    attention_body<HS, kAttF4, false, false, GEMMA, true>(a, h, pos0 + tok, smem, etab);
}

// ------------------------------------------------------------------------------------------------
// Multi-sequence pass (RowTable, lmrs_kernels.h): row r is one token of its own sequence, at its own position, over its own K / V cache.
// RoPE + scatter: rope_rows_kernel's rotation (the same four products, one difference and one sum per pair) on the rows of the qkv block, q in place,
// the key into the slot's blocked K cache, and the value row - which EPI_QKV would have stored itself - into the slot's V cache.
// ------------------------------------------------------------------------------------------------
// (one row of it: shared with the ragged pass's kernel below)
__device__ __forceinline__ void rope_scatter_row(float* row, float* k_slot, float* v_slot, const float* rope, int pos, int n_heads, int n_kv_heads, int hs,
                                                 int seq_len, int layer) {
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
            k_store_pair(k_slot + ((size_t)layer * n_kv_heads + kvh) * hs * (size_t)seq_len, seq_len, pos, j, half, rk.x, rk.y);
        }
    }
    const float4* v = reinterpret_cast<const float4*>(row + att + kv);                       // (att, kv multiples of 4: prefill_batched_ok)
    float4* vd = reinterpret_cast<float4*>(v_slot + ((size_t)layer * seq_len + pos) * kv);
    for (int i = threadIdx.x; i < kv / 4; i += blockDim.x) vd[i] = v[i];
}
__global__ __launch_bounds__(256) void rope_scatter_rows_kernel(float* qkv, float* k_cache, float* v_cache, const float* rope, const RowTable* rows,
                                                                 int n_heads, int n_kv_heads, int hs, int seq_len, int layer) {
    const int r = blockIdx.x;
    const size_t off = (size_t)rows->off[r];
    rope_scatter_row(qkv + (size_t)r * (n_heads + 2 * n_kv_heads) * hs, k_cache + off, v_cache + off, rope, rows->pos[r], n_heads, n_kv_heads, hs, seq_len, layer);
}
// the ragged pass (RowView): rows of one run share a slot at consecutive positions - distinct cache rows, so the order of the workgroups does not matter
__global__ __launch_bounds__(256) void rope_scatter_runs_kernel(float* qkv, float* k_cache, float* v_cache, const float* rope, const RowView rows,
                                                                 int n_heads, int n_kv_heads, int hs, int seq_len, int layer) {
    const int r = blockIdx.x;
    const size_t off = (size_t)rows.off[r];
    rope_scatter_row(qkv + (size_t)r * (n_heads + 2 * n_kv_heads) * hs, k_cache + off, v_cache + off, rope, rows.pos[r], n_heads, n_kv_heads, hs, seq_len, layer);
}

hipError_t launch_rope_scatter_rows(float* qkv, float* k_cache, float* v_cache, const float* rope, const RowTable* rows, int n_heads, int n_kv_heads, int hs,
                                    int seq_len, int layer, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRowTableMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rope_scatter_rows_kernel, dim3(n_rows), dim3(256), 0, s, qkv, k_cache, v_cache, rope, rows, n_heads, n_kv_heads, hs, seq_len, layer);
    return hipGetLastError();
}
hipError_t launch_rope_scatter_runs(float* qkv, float* k_cache, float* v_cache, const float* rope, RowView rows, int n_heads, int n_kv_heads, int hs,
                                    int seq_len, int layer, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRunRowsMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(rope_scatter_runs_kernel, dim3(n_rows), dim3(256), 0, s, qkv, k_cache, v_cache, rope, rows, n_heads, n_kv_heads, hs, seq_len, layer);
    return hipGetLastError();
}

// attention_rows_kernel over the table: grid (heads, rows); the workgroup takes its slot and position from its row and runs the same body.  The host
// has sorted the rows by descending position, so y = 0 is the deepest one.
template <int HS, bool GEMMA>
__device__ __forceinline__ void attention_table_row(const AttnArgs& a0, int r, size_t off, int pos, char* smem) {
    AttnArgs a = a0;
    const int h = blockIdx.x, att = a.n_heads * HS, kv = a.n_kv_heads * HS;
    a.q = a0.q + (size_t)r * (att + 2 * kv); a.out = a0.out + (size_t)r * att; a.dbg = nullptr;
    a.k_cache = a0.k_cache + off; a.v_cache = a0.v_cache + off;
    const uint64_t etab = exp2f_tab_lane();
    attention_body<HS, kAttF4, false, false, GEMMA, true>(a, h, pos, smem, etab);
}
template <int HS, bool GEMMA>
__global__ __launch_bounds__(kBlock) void attention_table_kernel(const AttnArgs a0, const RowTable* rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int r = blockIdx.y;
    attention_table_row<HS, GEMMA>(a0, r, (size_t)rows->off[r], rows->pos[r], smem);
}
// the ragged pass: the same workgroup per (head, row) over a RowView.  Row r of a run at position p reads keys 0 .. p of its slot - the rows of its own run
// at earlier positions among them, which rope_scatter_runs_kernel has stored before this launch starts; the later ones are never read.
template <int HS, bool GEMMA>
__global__ __launch_bounds__(kBlock) void attention_runs_kernel(const AttnArgs a0, const RowView rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int r = blockIdx.y;
    attention_table_row<HS, GEMMA>(a0, r, (size_t)rows.off[r], rows.pos[r], smem);
}

// the requested rows of a pass made consecutive (lmrs_batch_forward_runs' classifier runs over these only)
__global__ __launch_bounds__(256) void select_rows_kernel(const float* src, const uint32_t* sel, float* dst, int n4) {
    const float4* s = reinterpret_cast<const float4*>(src) + (size_t)sel[blockIdx.x] * n4;
    float4* d = reinterpret_cast<float4*>(dst) + (size_t)blockIdx.x * n4;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) d[i] = s[i];
}
hipError_t launch_select_rows(const float* src, const uint32_t* sel, float* dst, int n, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRunRowsMax || n % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(select_rows_kernel, dim3(n_rows), dim3(256), 0, s, src, sel, dst, n / 4);
    return hipGetLastError();
}

__global__ void table_advance_kernel(RowTable* rows, const uint32_t* idx, uint32_t* out, int n_rows) {
    const int r = threadIdx.x;
    if (r < n_rows) { const uint32_t t = idx[r]; out[r] = t; rows->tok[r] = t; rows->pos[r] += 1; }
}
hipError_t launch_table_advance(RowTable* rows, const uint32_t* idx, uint32_t* out, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRowTableMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(table_advance_kernel, dim3(1), dim3(64), 0, s, rows, idx, out, n_rows);
    return hipGetLastError();
}
// (the long table: the outputs are in the caller's row order, sel[o] is the table row behind output o - every row once)
__global__ void runs_advance_kernel(int* pos, uint32_t* tok, const uint32_t* sel, const uint32_t* idx, uint32_t* out, int n_rows) {
    const int o = threadIdx.x;
    if (o < n_rows) { const uint32_t t = idx[o], r = sel[o]; out[o] = t; tok[r] = t; pos[r] += 1; }
}
hipError_t launch_runs_advance(int* pos, uint32_t* tok, const uint32_t* sel, const uint32_t* idx, uint32_t* out, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(runs_advance_kernel, dim3(1), dim3(64), 0, s, pos, tok, sel, idx, out, n_rows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// The same attention for BLOCKS of 64 query tokens of one head (Llama / Phi): one lane per query.
// The per-(token, head) kernel above re-reads the whole K and V of its kv head for every query - 16 384 workgroups and
// ~2 GB of cache traffic per layer at 512 tokens; here a key or value row staged once serves 64 queries.  The reference's
// chains are kept per lane: the dot over the head dims of (query, key) is one chain, four keys interleaved for latency;
// the softmax sum one chain per query over its keys 0..p; out[d] one chain per (query, d) over the keys.  Scores / weights
// sit in a slab S[key][query] of global scratch per (head, block).  Causal attention makes the blocks unequal (the last
// block of a 512-token batch sees 8x the keys of the first), so the three phases are three launches, each cut the way ITS
// parallelism allows: scores by (block, 16 keys) - all independent; softmax by block with 16 waves sharing the order-free
// parts (max, exp, divide) around the one chain; values by (block, HS/8 output dims).
// Causality: a block works on the keys its LAST query sees; for an earlier query the later keys get weight 0.0 - their
// products +-0.0 are exact no-ops on a chain that starts at +0.0 - and are left out of its max and its sum.
// ------------------------------------------------------------------------------------------------
constexpr int kAttQB = 64;
size_t attention_block_scratch_floats(int n_heads, int n_tok, int T) { return (size_t)n_heads * ((n_tok + kAttQB - 1) / kAttQB) * (size_t)T * kAttQB; }

struct AttBlock { int i, p, T; bool live; };
__device__ __forceinline__ AttBlock att_block(int qb, int lane, int pos0, int n_tok) {
    AttBlock b;
    b.i = qb * kAttQB + lane; b.live = b.i < n_tok; b.i = b.live ? b.i : n_tok - 1;
    b.p = pos0 + b.i;                                                        // this lane's query position: keys 0..p
    const int last = qb * kAttQB + kAttQB - 1 < n_tok - 1 ? qb * kAttQB + kAttQB - 1 : n_tok - 1;
    b.T = pos0 + last + 1;                                                   // keys the block works on
    return b;
}

// scores (transformer.rs:507-516): workgroup = (64-key chunk, query block, head).  The 64 query rows and the 64 keys are staged
// once, coalesced, in LDS; lane l then holds query l in registers, wave w takes keys 16w .. 16w+15 (broadcast reads).
// kc: K cache of this layer; qrows: rotated queries [n_tok][att]
// UB dim groups of four staged keys (rows RS floats apart) -> registers; four score chains advanced over them
template <int UB, int RS>
__device__ __forceinline__ void att_kread(f32x4v (&k)[4][UB], const float* kr, int u0) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int u = 0; u < UB; ++u) k[j][u] = *reinterpret_cast<const f32x4v*>(kr + j * RS + (u0 + u) * 4);
}
template <int UB>
__device__ __forceinline__ void att_kdot(float& s0, float& s1, float& s2, float& s3, const f32x4v (&k)[4][UB], const f32x4v* q) {
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const f32x4v qq = q[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float pr;
            pr = qq[e] * k[0][u][e]; s0 = s0 + pr; pr = qq[e] * k[1][u][e]; s1 = s1 + pr;
            pr = qq[e] * k[2][u][e]; s2 = s2 + pr; pr = qq[e] * k[3][u][e]; s3 = s3 + pr;
        }
    }
}
// Staging of a score workgroup's 64 query rows and 64 keys in LDS (rows RS floats apart).  k_raw == nullptr: q is rotated already and every key sits in
// the cache (launch_rope_rows ran).  k_raw != nullptr (round 6: RoPE without a launch of its own, transformer.rs:443-495): q and the batch's keys arrive
// as the qkv GEMM left them; a thread takes a float4 of the first half of a head and its partner in the second half, rotates the pair with the position's
// (cos, sin) - the same four products, one difference and one sum per pair as rope_rows_kernel - and stages both; keys before pos0 come from the cache.
// `write_k` (one workgroup per kv head and key chunk: first head of the group, last query block - it sees every key): the rotated keys also go to
// the blocked K cache, for the value phase's successors (decode, the next batch).
template <int HS, int RS, int NK = 64, int NT = 256>             // NK: keys a workgroup stages (its chunk of the key axis); NT: its threads
__device__ __forceinline__ void att_stage(float* qt, float* kt, const float* __restrict__ qrows, const float* __restrict__ kT, float* kT_w, const float* __restrict__ k_raw,
                                          const float* __restrict__ rope, int att, int kv_dim, int h, int kvh, int qb, int cb, int bT, int n_tok, int pos0, int seq_len, bool write_k) {
    constexpr int HS4 = HS / 4, HS8 = HS / 8, half = HS / 2;
    const int tid = threadIdx.x;
    if (!k_raw) {
        for (int f = tid; f < 64 * HS4; f += NT) {
            const int r = f / HS4, c4 = f - r * HS4;                          // query row r: HS contiguous floats
            int qi = qb * kAttQB + r; qi = qi < n_tok ? qi : n_tok - 1;
            *reinterpret_cast<float4*>(qt + r * RS + c4 * 4) = *reinterpret_cast<const float4*>(qrows + (size_t)qi * att + h * HS + c4 * 4);
            if (NK == 64 || f < NK * HS4) {
                const int g = f / NK, kl = f % NK;                            // key kl, dim group g: consecutive keys 16 B apart
                const int key = cb + kl < bT ? cb + kl : bT - 1;
                *reinterpret_cast<float4*>(kt + kl * RS + g * 4) = *reinterpret_cast<const float4*>(kT + ((size_t)g * seq_len + key) * 4);
            }
        }
        return;
    }
    auto rotate = [](const float4& v0, const float4& v1, const float4& r0, const float4& r1, float4& o0, float4& o1) __attribute__((always_inline)) {
        // r0 = (cos0, sin0, cos1, sin1), r1 = (cos2, sin2, cos3, sin3) of the pair's four dims
        float a0, a1, b0, b1;
        a0 = v0.x * r0.x; a1 = v1.x * r0.y; b0 = v0.x * r0.y; b1 = v1.x * r0.x; o0.x = a0 - a1; o1.x = b0 + b1;
        a0 = v0.y * r0.z; a1 = v1.y * r0.w; b0 = v0.y * r0.w; b1 = v1.y * r0.z; o0.y = a0 - a1; o1.y = b0 + b1;
        a0 = v0.z * r1.x; a1 = v1.z * r1.y; b0 = v0.z * r1.y; b1 = v1.z * r1.x; o0.z = a0 - a1; o1.z = b0 + b1;
        a0 = v0.w * r1.z; a1 = v1.w * r1.w; b0 = v0.w * r1.w; b1 = v1.w * r1.z; o0.w = a0 - a1; o1.w = b0 + b1;
    };
    const bool any_raw = cb + NK - 1 >= pos0, any_cached = cb < pos0;        // (both only in the one chunk pos0 falls into)
    for (int f = tid; f < 64 * HS8; f += NT) {
        const int r = f / HS8, c = f - r * HS8;                              // row r, dims 4c .. 4c+3 and their partners half further on
        {
            int qi = qb * kAttQB + r; qi = qi < n_tok ? qi : n_tok - 1;
            const float* qp = qrows + (size_t)qi * att + h * HS + c * 4;
            const float* rp = rope + ((size_t)(pos0 + qi) * half + c * 4) * 2;
            const float4 v0 = *reinterpret_cast<const float4*>(qp), v1 = *reinterpret_cast<const float4*>(qp + half);
            const float4 r0 = *reinterpret_cast<const float4*>(rp), r1 = *reinterpret_cast<const float4*>(rp + 4);
            float4 o0, o1; rotate(v0, v1, r0, r1, o0, o1);
            *reinterpret_cast<float4*>(qt + r * RS + c * 4) = o0; *reinterpret_cast<float4*>(qt + r * RS + half + c * 4) = o1;
        }
        if (any_raw && (NK == 64 || r < NK)) {
            const bool real = cb + r < bT;
            const int key = real ? cb + r : bT - 1;
            if (key >= pos0) {
                const float* kp = k_raw + (size_t)(key - pos0) * kv_dim + kvh * HS + c * 4;
                const float* rp = rope + ((size_t)key * half + c * 4) * 2;
                const float4 v0 = *reinterpret_cast<const float4*>(kp), v1 = *reinterpret_cast<const float4*>(kp + half);
                const float4 r0 = *reinterpret_cast<const float4*>(rp), r1 = *reinterpret_cast<const float4*>(rp + 4);
                float4 o0, o1; rotate(v0, v1, r0, r1, o0, o1);
                *reinterpret_cast<float4*>(kt + r * RS + c * 4) = o0; *reinterpret_cast<float4*>(kt + r * RS + half + c * 4) = o1;
                if (write_k && real) {
                    *reinterpret_cast<float4*>(kT_w + ((size_t)c * seq_len + key) * 4) = o0;
                    *reinterpret_cast<float4*>(kT_w + ((size_t)(c + HS8) * seq_len + key) * 4) = o1;
                }
            }
        }
    }
    if (any_cached) {
        for (int f = tid; f < NK * HS4; f += NT) {
            const int g = f / NK, kl = f % NK;
            const int key = cb + kl < bT ? cb + kl : bT - 1;
            if (key < pos0) *reinterpret_cast<float4*>(kt + kl * RS + g * 4) = *reinterpret_cast<const float4*>(kT + ((size_t)g * seq_len + key) * 4);
        }
    }
}
template <int HS>
__global__ __launch_bounds__(256) void att_scores_kernel(const float* __restrict__ qrows, float* kc, float* __restrict__ scratch, const float* __restrict__ k_raw,
                                                         const float* __restrict__ rope, int n_heads, int n_kv_heads, int seq_len, int pos0, int n_tok, int Tmax) {
    constexpr int RS = HS + 4, HS4 = HS / 4;
    __shared__ __attribute__((aligned(16))) float qt[64 * RS];
    __shared__ __attribute__((aligned(16))) float kt[64 * RS];
    // grid (head, key chunk, query block): the HEAD is the fastest index - workgroup b lands on XCD b % 8, and with the chunk (or the
    // query block) fastest the causal triangle put all the heavy workgroups on one XCD and all the empty ones on another
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), qb = gridDim.z - 1 - blockIdx.z, h = blockIdx.x;   // (the last query blocks, with the most keys, are dispatched first)
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    const int cb = blockIdx.y * 64;
    if (cb >= b.T) return;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul, att = n_heads * HS;
    float* S = scratch + ((size_t)h * gridDim.z + qb) * (size_t)Tmax * kAttQB + lane;    // S[key * 64]
    float* kT = kc + (size_t)kvh * HS * (size_t)seq_len;                                 // [HS/4][seq][4]
    att_stage<HS, RS>(qt, kt, qrows, kT, kT, k_raw, rope, att, n_kv_heads * HS, h, kvh, qb, cb, b.T, n_tok, pos0, seq_len, h % kv_mul == 0 && qb == (int)gridDim.z - 1);
    __syncthreads();
    const int c0 = cb + wave * 16;
    if (c0 >= b.T) return;
    const int nk = b.T - c0 < 16 ? b.T - c0 : 16;
    f32x4v q[HS4];
#pragma unroll
    for (int u = 0; u < HS4; ++u) q[u] = *reinterpret_cast<const f32x4v*>(qt + lane * RS + u * 4);
    const float sqrt_hs = sqrtf((float)HS);
    const float* kv = kt + wave * 16 * RS;
    constexpr int UB = 2;                                                    // dim groups per batch of LDS reads (4 keys each)
    static_assert(HS4 % (2 * UB) == 0, "head size");
#pragma unroll 1
    for (int kk = 0; kk < nk; kk += 4) {                                     // rows nk.. hold the (valid) clamped key: computed, not stored
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
            if (kk + j < nk) S[(size_t)(c0 + kk + j) * kAttQB] = sc[j];      // wave-uniform
    }
}

// The same for Gemma-2's 256-wide heads (transformer.rs:507-526): a lane cannot hold a 256-float query row next to the staged keys, and the chain over
// the head dims may not be cut - so the dims are walked in TWO passes of 128 with the query half in registers, the 16 partial sums of the wave's 16 keys
// carried from the first pass to the second (same chain, same order).  Then the soft-cap - score / 50, f64 tanh, * 50 - and the window term with the
// reference's u32 arithmetic on the FIRST position of the forward_layer call (st->win_base: the quirk attention_body documents) - or, when the pass
// stands for n forward calls (win_base == kWinPerQuery), on each query's OWN position, which is what the decode step tests.
template <int HS, int NK, int NT>
__global__ __launch_bounds__(NT) void att_scores_wide_kernel(const float* __restrict__ qrows, float* kc, float* __restrict__ scratch, const DevState* __restrict__ st, const float* __restrict__ k_raw,
                                                              const float* __restrict__ rope, int n_heads, int n_kv_heads, int seq_len, int pos0, int n_tok, int Tmax) {
    constexpr int HP = HS / 2, RS = HS + 4, HP4 = HP / 4;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* qt = reinterpret_cast<float*>(smem_raw);              // [64][RS]
    float* kt = qt + 64 * RS;                                    // [NK][RS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), qb = gridDim.z - 1 - blockIdx.z, h = blockIdx.x;
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    constexpr int KW = NK / (NT / 64);                           // keys per wave
    static_assert(KW % 4 == 0 && KW >= 4, "four score chains at a time");
    const int cb = blockIdx.y * NK;
    if (cb >= b.T) return;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul, att = n_heads * HS;
    float* S = scratch + ((size_t)h * gridDim.z + qb) * (size_t)Tmax * kAttQB + lane;
    float* kT = kc + (size_t)kvh * HS * (size_t)seq_len;                                 // [HS/4][seq][4]
    att_stage<HS, RS, NK, NT>(qt, kt, qrows, kT, kT, k_raw, rope, att, n_kv_heads * HS, h, kvh, qb, cb, b.T, n_tok, pos0, seq_len, h % kv_mul == 0 && qb == (int)gridDim.z - 1);
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
            if (kq * 4 < nk) {                                               // wave-uniform; keys nk.. hold the (valid) clamped key: computed, not stored
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
        if (i < nk) {                                                        // wave-uniform
            const int t = c0 + i;
            S[(size_t)t * kAttQB] = gemma_cap_window(part[i] / sqrt_hs, wpos, t);
        }
    }
}

// softmax (functional.rs:122-140) of 16 queries of a block over their keys 0..p.  exp dominates the arithmetic (one per (query, key),
// ~60 instructions of f64 work) and the sum is one chain per query, so a block is cut into four workgroups of 16 queries:
// lane = (query q, key phase ph), 4 waves x 8 x 4 phases = 128 keys per sweep (small workgroups: all of them resident at once).  max, exp and divide are order-free and shared
// by all lanes; the chain runs in wave 0 over exponentials already masked to +0.0 past p (exact on a sum >= +0) - pure adds.
// IN_LDS (T <= kAttLdsKeys, lmrs_switches.h): the scores live in LDS between the passes - the chain reads LDS, not memory.
constexpr int kAttSQ = 16, kAttSW = 4;                                      // queries and waves per softmax workgroup
template <bool IN_LDS>
__global__ __launch_bounds__(kAttSW * 64) void att_softmax_kernel(int pos0, int n_tok, float* scratch, int Tmax) {
    constexpr int SWEEP = kAttSW * 32;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* red = reinterpret_cast<float*>(smem_raw);                         // [waves][64 lanes]
    float* rowsum = red + kAttSW * 64;                                       // [16]
    float* E = rowsum + kAttSQ;                                              // IN_LDS: [T + 48][16]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h = blockIdx.x, q0 = blockIdx.z * kAttSQ;
    // head fastest (workgroup b lands on XCD b % 8: every XCD gets every block length); the workgroups that end up sharing a CU are 256 apart
    // in dispatch order, i.e. the same (head, block) of the next query quarter: alternate quarters walk the blocks in opposite directions,
    // so that a long block shares its CU with a short one
    const int qb = (blockIdx.z & 1) ? (int)blockIdx.y : (int)(gridDim.y - 1 - blockIdx.y);

    const int q = lane & 15, ph = lane >> 4;
    const AttBlock b = att_block(qb, q0 + q, pos0, n_tok);
    const int T = b.T, p = b.p;
    const uint64_t etab = exp2f_tab_lane();
    float* S = scratch + ((size_t)h * gridDim.y + qb) * (size_t)Tmax * kAttQB + q0 + q;
    float* EL = E + q;
    // lane's keys of a sweep starting at kb: kb + wave * 32 + u * 4 + ph, u = 0..7 (wave-uniform trip count: expf shuffles across the wave)
    float mx = __uint_as_float(0xff800000u);
    for (int kb = wave * 32; kb < T; kb += SWEEP) {
        const int k0 = kb + ph;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * 4; v[u] = S[(size_t)(k < T ? k : T - 1) * kAttQB]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + u * 4;
            mx = (k <= p && k < T) ? fmaxf(mx, v[u]) : mx;
            if (IN_LDS && k < T) EL[k * kAttSQ] = v[u];
        }
    }
    red[wave * 64 + lane] = mx;
    __syncthreads();
    mx = red[q];
    for (int w = 1; w < kAttSW * 4; ++w) mx = fmaxf(mx, red[w * 16 + q]);    // waves x 4 phases of query q
    for (int kb = wave * 32; kb < T; kb += SWEEP) {
        const int k0 = kb + ph;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { int k = k0 + u * 4; k = k < T ? k : T - 1; v[u] = IN_LDS ? EL[k * kAttSQ] : S[(size_t)k * kAttQB]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = expf_glibc_t(v[u] - mx, etab);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + u * 4;
            const float e = (k <= p) ? v[u] : 0.0f;                          // past p: +0.0, an exact no-op in the sum and 0.0 after the divide
            if (k < T) { if (IN_LDS) EL[k * kAttSQ] = e; else S[(size_t)k * kAttQB] = e; }
        }
    }
    if (IN_LDS) for (int f = threadIdx.x; f < 48 * kAttSQ; f += kAttSW * 64) E[T * kAttSQ + f] = 0.0f;   // +0.0 rows T .. T+47: the chain runs in whole batches, one batch read ahead
    __syncthreads();                                                          // (also drains the S stores: hipcc's barrier waits for vmcnt(0))
    if (wave == 0 && ph == 0) {
        float sum = 0.0f;
        if constexpr (IN_LDS) {                                              // batches of 16, the next batch's reads ahead of the adds
            float va[16], vb[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) va[u] = EL[u * kAttSQ];
            for (int k = 0; k < T; k += 32) {
#pragma unroll
                for (int u = 0; u < 16; ++u) vb[u] = EL[(k + 16 + u) * kAttSQ];
#pragma unroll
                for (int u = 0; u < 16; ++u) sum = sum + va[u];
                asm volatile("" : "+v"(sum) : : "memory");
                if (k + 16 < T) {
#pragma unroll
                    for (int u = 0; u < 16; ++u) va[u] = EL[(k + 32 + u) * kAttSQ];
#pragma unroll
                    for (int u = 0; u < 16; ++u) sum = sum + vb[u];
                    asm volatile("" : "+v"(sum) : : "memory");
                }
            }
        } else {
            for (int k = 0; k < T; ++k) sum = sum + S[(size_t)k * kAttQB];
        }
        rowsum[q] = sum;
    }
    __syncthreads();
    const float sum = rowsum[q];
    for (int kb = wave * 32; kb < T; kb += SWEEP) {
        const int k0 = kb + ph;
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { int k = k0 + u * 4; k = k < T ? k : T - 1; v[u] = IN_LDS ? EL[k * kAttSQ] : S[(size_t)k * kAttQB]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int k = k0 + u * 4; if (k < T) S[(size_t)k * kAttQB] = v[u] / sum; }
    }
}

// weighted sum of values (transformer.rs:533-541): workgroup = (query block, head, slice of NW * DW output dims), wave w owns DW of
// them, one chain per (lane, dim) over the keys.  Tiles of 64 keys - the weights S[key][query] and the value row slices - are
// loaded by the whole workgroup one tile ahead (registers) and consumed from double-buffered LDS: one barrier per tile.  A value
// is the same for all 64 lanes: a broadcast LDS read costs what a full one does (2 cycles per dword and wave), which is what
// bounds this phase - hence the split of a block's dims over several workgroups (and so CUs).
// vc: V cache of this layer [seq][kv_dim]
template <int NT, int SW, int NS, int NV>                                    // SW: dims of the slice; NS / NV: float4 per thread of the weight / value tile
__device__ __forceinline__ void att_tile_load(f32x4v (&rw)[NS], f32x4v (&rv)[NV], const float* Sb, const float* vb, int kv_dim, int t, int T) {
    constexpr int SW4 = SW / 4;
    const int tid = threadIdx.x, k0 = t * 64;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int f = tid + j * NT, kl = f >> 4, c4 = f & 15;
        const int key = k0 + kl < T ? k0 + kl : T - 1;
        const f32x4v w4 = *reinterpret_cast<const f32x4v*>(Sb + (size_t)key * kAttQB + c4 * 4);
        rw[j] = k0 + kl < T ? w4 : f32x4v{0.0f, 0.0f, 0.0f, 0.0f};           // rows past the last key: weight 0.0 (their +-0.0 products are exact no-ops)
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int f = tid + j * NT;
        if (NV * NT == 64 * SW4 || f < 64 * SW4) {
            const int kl = f / SW4, c4 = f - kl * SW4;
            const int key = k0 + kl < T ? k0 + kl : T - 1;
            rv[j] = *reinterpret_cast<const f32x4v*>(vb + (size_t)key * kv_dim + c4 * 4);
        }
    }
}
template <int NT, int SW, int NS, int NV>
__device__ __forceinline__ void att_tile_store(const f32x4v (&rw)[NS], const f32x4v (&rv)[NV], float* dst) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NS; ++j) { const int f = tid + j * NT; *reinterpret_cast<f32x4v*>(dst + f * 4) = rw[j]; }
#pragma unroll
    for (int j = 0; j < NV; ++j) { const int f = tid + j * NT; if (NV * NT == 16 * SW || f < 16 * SW) *reinterpret_cast<f32x4v*>(dst + 64 * 64 + f * 4) = rv[j]; }
}
template <int HS, int DW, int SW>
__device__ __forceinline__ void att_tile_compute(float (&acc)[DW], const float* cur, int lane, int wave, int left) {
    const float* wl = cur + lane;
    const float* vl = cur + 64 * 64 + wave * DW;
    const int nk = left < 64 ? left : 64;
    for (int k8 = 0; k8 < nk; k8 += 8) {                                     // whole batches of 8: no branch between a row's reads and its adds
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = wl[(k8 + u) * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4* vr = reinterpret_cast<const float4*>(vl + (k8 + u) * SW);
#pragma unroll
            for (int g = 0; g < DW / 4; ++g) {
                const float4 vv = vr[g];
                float pr;
                pr = w[u] * vv.x; acc[g * 4 + 0] = acc[g * 4 + 0] + pr; pr = w[u] * vv.y; acc[g * 4 + 1] = acc[g * 4 + 1] + pr;
                pr = w[u] * vv.z; acc[g * 4 + 2] = acc[g * 4 + 2] + pr; pr = w[u] * vv.w; acc[g * 4 + 3] = acc[g * 4 + 3] + pr;
            }
        }
    }
}
template <int HS, int NW, int DW>
__global__ __launch_bounds__(NW * 64) void att_values_kernel(const float* __restrict__ vc, const float* __restrict__ scratch, float* __restrict__ out,
                                                             int n_heads, int n_kv_heads, int pos0, int n_tok, int Tmax) {
    constexpr int NT = NW * 64, SW = NW * DW, NS = 64 * 16 / NT, NV = (16 * SW + NT - 1) / NT;
    static_assert(HS % SW == 0 && DW % 4 == 0 && (64 * 16) % NT == 0, "slice geometry");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);                          // 2 x { weights [64][64], values [64][SW] }
    constexpr int TILE = 64 * 64 + 64 * SW;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = blockIdx.x, sl = blockIdx.z;
    // head fastest (XCD balance); the two dim slices walk the query blocks in opposite directions: the workgroups that share a CU (256 apart in
    // dispatch order) are then a long block and a short one, not two long ones
    const int qb = (sl & 1) ? (int)blockIdx.y : (int)(gridDim.y - 1 - blockIdx.y);
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    const int T = b.T, n_tiles = (T + 63) / 64;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul, kv_dim = n_kv_heads * HS, att = n_heads * HS;
    const float* Sb = scratch + ((size_t)h * gridDim.y + qb) * (size_t)Tmax * kAttQB;
    const float* vb = vc + kvh * HS + sl * SW;
    // two register sets, each loaded two tile-computes before it is stored to LDS (a first-touch read of the slab comes from
    // memory, ~2 us: the previous launch's L2 does not survive); LDS double-buffered, one barrier per tile
    f32x4v rwa[NS], rva[NV], rwb[NS], rvb[NV];
    float acc[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) acc[d] = 0.0f;
    att_tile_load<NT, SW, NS, NV>(rwa, rva, Sb, vb, kv_dim, 0, T);
    att_tile_store<NT, SW, NS, NV>(rwa, rva, sm);
    // (the prefetches are unconditional - a tile past the end re-reads the last key with weight 0 and is never stored: a load under
    // a branch makes hipcc wait for every outstanding load at the join, the ones issued for later tiles included)
    att_tile_load<NT, SW, NS, NV>(rwa, rva, Sb, vb, kv_dim, 1, T);
    att_tile_load<NT, SW, NS, NV>(rwb, rvb, Sb, vb, kv_dim, 2, T);
    lds_barrier();
    for (int t = 0; t < n_tiles; t += 2) {
        att_tile_compute<HS, DW, SW>(acc, sm, lane, wave, T - t * 64);
        if (t + 1 < n_tiles) att_tile_store<NT, SW, NS, NV>(rwa, rva, sm + TILE);
        att_tile_load<NT, SW, NS, NV>(rwa, rva, Sb, vb, kv_dim, t + 3, T);
        lds_barrier();                                                       // (not __syncthreads: that would drain the loads just issued)
        if (t + 1 < n_tiles) {
            att_tile_compute<HS, DW, SW>(acc, sm + TILE, lane, wave, T - (t + 1) * 64);
            if (t + 2 < n_tiles) att_tile_store<NT, SW, NS, NV>(rwb, rvb, sm);
            att_tile_load<NT, SW, NS, NV>(rwb, rvb, Sb, vb, kv_dim, t + 4, T);
            lds_barrier();
        }
    }
    if (b.live) {
        float* ob = out + (size_t)b.i * att + h * HS + sl * SW + wave * DW;
#pragma unroll
        for (int g = 0; g < DW / 4; ++g) *reinterpret_cast<float4*>(ob + g * 4) = make_float4(acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]);
    }
}

bool attention_block_supported(const AttnArgs& a, int n_tok) {
    if (a.gemma) return n_tok >= 16 && a.head_size == 256 && a.n_heads % a.n_kv_heads == 0;
    return n_tok >= 16 && (a.head_size == 64 || a.head_size == 96 || a.head_size == 128) && a.n_heads % a.n_kv_heads == 0;
}

// lds_keys: longest context whose scores stay in LDS (LMRS_ATT_LDS_KEYS); long_forms: Gemma-2's long-batch forms at any length (LMRS_ATT_LONG_BATCH_FORMS)
hipError_t launch_attention_block(const AttnArgs& a, int pos0, int n_tok, float* scratch, int lds_keys, bool long_forms, hipStream_t s) {
    const int T = pos0 + n_tok, nqb = (n_tok + kAttQB - 1) / kAttQB, nch = (T + 63) / 64;
    const int kv_dim = a.n_kv_heads * a.head_size;
    float* kc = a.k_cache + (size_t)a.layer * kv_dim * (size_t)a.seq_len;
    const float* kraw = a.k_raw; const float* rope = a.k_raw ? a.rope : nullptr;          // k_raw set: RoPE folded into the score kernel's staging (att_stage)
    const float* vc = a.v_cache + (size_t)a.layer * a.seq_len * kv_dim;
    const bool in_lds = T <= lds_keys;
    const size_t sm = (kAttSW * 64 + kAttSQ + (in_lds ? (size_t)(T + 48) * kAttSQ : 0)) * sizeof(float);
    allow_big_lds(reinterpret_cast<const void*>(att_softmax_kernel<true>));
#define AB(HS_, NW_, DW_)                                                                                                             \
    {                                                                                                                                 \
        hipLaunchKernelGGL((att_scores_kernel<HS_>), dim3(a.n_heads, nch, nqb), dim3(256), 0, s, a.q, kc, scratch, kraw, rope, a.n_heads, a.n_kv_heads, a.seq_len, pos0, n_tok, T); \
        if (in_lds) hipLaunchKernelGGL(att_softmax_kernel<true>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);    \
        else hipLaunchKernelGGL(att_softmax_kernel<false>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);          \
        allow_big_lds(reinterpret_cast<const void*>(att_values_kernel<HS_, NW_, DW_>));                                                   \
        hipLaunchKernelGGL((att_values_kernel<HS_, NW_, DW_>), dim3(a.n_heads, nqb, HS_ / (NW_ * DW_)), dim3(NW_ * 64), 2 * (64 * 64 + 64 * NW_ * DW_) * sizeof(float), s, \
                           vc, (const float*)scratch, a.out, a.n_heads, a.n_kv_heads, pos0, n_tok, T);                                  \
        return hipGetLastError();                                                                                                     \
    }
    if (a.gemma) {                                                            // 256-wide heads, soft-capped scores (att_scores_wide_kernel)
        if (a.head_size != 256) return hipErrorInvalidValue;
        // Workgroup = (head, key chunk, query block): with 8 heads a 64-key chunk leaves most of the chip idle up to a few hundred tokens (256 tokens: 80 live
        // workgroups, each wave walking 16 keys x 256 dims alone: 35 us per layer).  Round 6: 32-key chunks and 8 waves of 4 keys while the 64-key grid would not
        // give every CU two workgroups - twice the workgroups, a quarter of the keys per wave.
        int live64 = 0;
        for (int qb = 0; qb < nqb; ++qb) { const int last = qb * kAttQB + kAttQB - 1 < n_tok - 1 ? qb * kAttQB + kAttQB - 1 : n_tok - 1; live64 += (pos0 + last + 1 + 63) / 64; }
        live64 *= a.n_heads;
        if (live64 < 512 && !long_forms) {
            constexpr size_t smem32 = (size_t)(64 + 32) * (256 + 4) * sizeof(float);
            allow_big_lds(reinterpret_cast<const void*>(att_scores_wide_kernel<256, 32, 512>));
            hipLaunchKernelGGL((att_scores_wide_kernel<256, 32, 512>), dim3(a.n_heads, (T + 31) / 32, nqb), dim3(512), smem32, s, a.q, kc, scratch, a.st, kraw, rope, a.n_heads, a.n_kv_heads, a.seq_len, pos0, n_tok, T);
        } else {
            constexpr size_t wide_smem = (size_t)2 * 64 * (256 + 4) * sizeof(float);
            allow_big_lds(reinterpret_cast<const void*>(att_scores_wide_kernel<256, 64, 256>));
            hipLaunchKernelGGL((att_scores_wide_kernel<256, 64, 256>), dim3(a.n_heads, nch, nqb), dim3(256), wide_smem, s, a.q, kc, scratch, a.st, kraw, rope, a.n_heads, a.n_kv_heads, a.seq_len, pos0, n_tok, T);
        }
        if (in_lds) hipLaunchKernelGGL(att_softmax_kernel<true>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);
        else hipLaunchKernelGGL(att_softmax_kernel<false>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);
        if (a.n_heads * nqb * 4 < 256 && !long_forms) {                                      // (few blocks: 32-dim slices - twice the workgroups, 4 dims per wave as for the 64-wide heads)
            allow_big_lds(reinterpret_cast<const void*>(att_values_kernel<256, 8, 4>));
            hipLaunchKernelGGL((att_values_kernel<256, 8, 4>), dim3(a.n_heads, nqb, 256 / 32), dim3(512), 2 * (64 * 64 + 64 * 32) * sizeof(float), s,
                               vc, (const float*)scratch, a.out, a.n_heads, a.n_kv_heads, pos0, n_tok, T);
            return hipGetLastError();
        }
        allow_big_lds(reinterpret_cast<const void*>(att_values_kernel<256, 8, 8>));
        hipLaunchKernelGGL((att_values_kernel<256, 8, 8>), dim3(a.n_heads, nqb, 256 / 64), dim3(512), 2 * (64 * 64 + 64 * 64) * sizeof(float), s,
                           vc, (const float*)scratch, a.out, a.n_heads, a.n_kv_heads, pos0, n_tok, T);
        return hipGetLastError();
    }
    switch (a.head_size) { case 64: AB(64, 8, 4) case 96: AB(96, 4, 12) case 128: AB(128, 8, 8) default: return hipErrorInvalidValue; }
#undef AB
}

hipError_t launch_attention_rows(const AttnArgs& a0, int pos0, int n_tok, hipStream_t s) {
    AttnArgs a = a0;
    // Thousands of independent (head, token) workgroups: a small LDS footprint (64-row V chunks, the score array sized for the
    // longest sequence of THIS batch instead of seq_len) lets several of them share a CU.
    a.chunk = 64;
    if (a.chunk * (a.head_size / 4) > kAttF4 * kBlock) return hipErrorInvalidValue;
    const size_t smem = attention_smem(a.head_size, a.chunk, pos0 + n_tok);
#define AR(HS_, G_)                                                                                                                   \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(attention_rows_kernel<HS_, G_>));                                                 \
        hipLaunchKernelGGL((attention_rows_kernel<HS_, G_>), dim3(a.n_heads, n_tok), dim3(kBlock), smem, s, a, pos0);                  \
        return hipGetLastError();                                                                                                     \
    }
    if (a.gemma) { if (a.head_size == 256) AR(256, true) return hipErrorInvalidValue; }
    switch (a.head_size) { case 64: AR(64, false) case 96: AR(96, false) case 128: AR(128, false) default: return hipErrorInvalidValue; }
#undef AR
}

hipError_t launch_attention_table(const AttnArgs& a0, const RowTable* rows, int n_rows, int max_T, hipStream_t s) {
    AttnArgs a = a0;
    a.chunk = 64;                                                          // as launch_attention_rows: the small LDS footprint
    if (n_rows < 1 || n_rows > kRowTableMax || max_T < 1 || max_T > a.seq_len || a.chunk * (a.head_size / 4) > kAttF4 * kBlock) return hipErrorInvalidValue;
    const size_t smem = attention_smem(a.head_size, a.chunk, max_T);
#define AT(HS_, G_)                                                                                                                   \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(attention_table_kernel<HS_, G_>));                                                \
        hipLaunchKernelGGL((attention_table_kernel<HS_, G_>), dim3(a.n_heads, n_rows), dim3(kBlock), smem, s, a, rows);                \
        return hipGetLastError();                                                                                                     \
    }
    if (a.gemma) { if (a.head_size == 256) AT(256, true) return hipErrorInvalidValue; }
    switch (a.head_size) { case 64: AT(64, false) case 96: AT(96, false) case 128: AT(128, false) default: return hipErrorInvalidValue; }
#undef AT
}

// launch_attention_table over a RowView of up to kRunRowsMax rows
hipError_t launch_attention_runs(const AttnArgs& a0, RowView rows, int n_rows, int max_T, hipStream_t s) {
    AttnArgs a = a0;
    a.chunk = 64;
    if (n_rows < 1 || n_rows > kRunRowsMax || max_T < 1 || max_T > a.seq_len || a.chunk * (a.head_size / 4) > kAttF4 * kBlock) return hipErrorInvalidValue;
    const size_t smem = attention_smem(a.head_size, a.chunk, max_T);
#define AT(HS_, G_)                                                                                                                   \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(attention_runs_kernel<HS_, G_>));                                                 \
        hipLaunchKernelGGL((attention_runs_kernel<HS_, G_>), dim3(a.n_heads, n_rows), dim3(kBlock), smem, s, a, rows);                 \
        return hipGetLastError();                                                                                                     \
    }
    if (a.gemma) { if (a.head_size == 256) AT(256, true) return hipErrorInvalidValue; }
    switch (a.head_size) { case 64: AT(64, false) case 96: AT(96, false) case 128: AT(128, false) default: return hipErrorInvalidValue; }
#undef AT
}
