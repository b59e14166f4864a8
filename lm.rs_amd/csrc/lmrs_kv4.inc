// ------------------------------------------------------------------------------------------------
// The table pass over paged K/V kept in 4 BITS (lmrs_batch_create_paged_q4; included by lmrs_kernels.hip behind lmrs_kvq.inc).
// The rule: every K row (after RoPE) and every V row is stored in groups of 32 consecutive elements of the kv_dim row, each group quantised by the
// reference's Q4_0 rule (quantization.rs:69-95 with a group of 32), operation for operation:
//   scale  = max|x| / -8.0f                       NEGATIVE, the reference's doing
//   nibble = clamp(sat_u8(round_half_away(x / scale + 8.0f)), 0, 15)      a division per element, the sum rounded on its own; sat_u8: Rust's `as u8`,
//                                                 below 0 -> 0, NaN -> 0 (quant_q4 writes the saturation out; no cast decides it)
//   elements 2i and 2i + 1 share a byte, low nibble first
// and a cached value reads back as (float)(nibble - 8) * scale, one rounding (quantization.rs:17-23, :32-39).  What follows from it: an all-zero group has
// scale -0.0, every nibble 0 and reads back as +0.0; a zero inside a non-zero group is nibble 8 and reads back as -0.0; +max reads back exactly, -max
// as -7/8 max (nibble 15); a group whose maximum is denormal has scale -0.0 and reads back as +-0.0; maxima of 3e38 stay finite.  A page of all-zero
// bytes (the zero page, a page cleared at its claim) is nibble 0 times scale +0.0 = -0.0: "a position nobody wrote reads as zero" holds as a NUMERIC
// statement (the row compares equal to 0.0, it is not the bit pattern of +0.0).
// A row at position p attends to keys and values 0 .. p-1 as read back and to its OWN key and value in f32, as the pass computed them (the rotated k
// and the v of its qkv row).  Everything else is paged_attention_body's operations in the same order per value.
// A page (page_bytes apart, K block first, V block page_bytes / 2 behind; nib_bytes = n_layers * page_len * kv_dim / 2).  One 16-byte word is a WHOLE
// group - 32 dims of one key - so the unit of every layout below is the group:
//   K nibbles [layer][kv head][hs / 32][page_len][16]   a score lane's batch is ONE 16-byte load and one scale, five registers in flight where Q8 holds
//                                                       nine; a wave's 64 loads are 1024 consecutive bytes
//   K scales  [layer][kv head][hs / 32][page_len]       f32, nib_bytes behind the K block's start; a wave's 64 loads are 256 consecutive bytes
//   V nibbles [layer][kv head][page_len][hs / 2]        HEAD-MAJOR, unlike the Q8 pages' [layer][page_len][kv_dim]: a workgroup stages 64 rows of ONE kv
//   V scales  [layer][kv head][page_len][hs / 32]       head, and at 4 bits a head's share of a kv_dim row is 32 .. 128 bytes - a fraction of a 128-byte
//                                                       line, the rest of it other heads' values.  Head-major, the chunk's 64 rows are 64 * hs / 2
//                                                       consecutive bytes (2 .. 8 KiB) and its scales 64 * hs / 8: every line that is read is used whole,
//                                                       lane after lane 8 bytes on
// 0.625 bytes a cached value: 20 bytes a group of 32.
// What was built: ONE WORKGROUP PER (HEAD, ROW), as kvq_attn_kernel and paged_attn_kernel.  The (kv head, row) split - a key unpacked once for its
// kv_mul query heads - was not built or measured.  A prompt chunk of ONE slot of kKv4BlockMin rows or more (lmrs_api.hip) takes BLOCK attention over
// the same pages (the second half of this file: block_kv4_scores_kernel, block_kv4_scores_wide_kernel, block_kv4_values_kernel); shorter chunks,
// ragged runs and decode rows take the table pass.
// Out of scope: a block floor below 320 rows, Q4 for contiguous and wide batches or the context's own cache, mixed K / V formats.
// ------------------------------------------------------------------------------------------------
typedef int i32x2v __attribute__((ext_vector_type(2)));
// built without the packed f32 instructions, as the Q8 kernels are and for their reason (lmrs_kvq.inc): every value is compared bit for bit
#if defined(__HIP_DEVICE_COMPILE__)
#define KV4_KERNEL __global__ __attribute__((target("no-packed-fp32-ops")))
#else
#define KV4_KERNEL __global__
#endif

// ---- the two device functions of the format: the quantiser of the stores and the read-back of the loads (lmrs_op_kv4_round_trip runs these two)
// Eight consecutive elements of a row in this lane, a group of 32 in an aligned cluster of 4 lanes - the group maximum is two DPP steps: the group's
// scale, this lane's eight nibbles as one word.  m / -8.0f is exact up to the one rounding a denormal quotient takes (the reference's own); 0 / -0.0 =
// NaN and x / -0.0 = -+inf land on nibbles 0, 0 and 15 through quant_q4's written-out saturation.
__device__ __forceinline__ uint32_t kv4_quant8(const float4 a, const float4 b, float& scale) {
    const float m = cluster_max<4>(absmax4(b, absmax4(a, 0.0f)));
    scale = m / -8.0f;
    return quant_q4(a.x, scale) | quant_q4(a.y, scale) << 4 | quant_q4(a.z, scale) << 8 | quant_q4(a.w, scale) << 12 |
           quant_q4(b.x, scale) << 16 | quant_q4(b.y, scale) << 20 | quant_q4(b.z, scale) << 24 | quant_q4(b.w, scale) << 28;
}
// A word of eight nibbles read back: dims 0 .. 3 in `a`, 4 .. 7 in `b`.  The low and the high nibbles are masked out ONCE per word (three integer
// operations for eight values), each then a byte of its own - a byte-to-float conversion (v_cvt_f32_ubyteN) needs no shift.  Per value: the
// conversion, - 8.0f (exact: integers 0 .. 15), * scale (the rule's one rounding) - three operations where a Q8 value takes two.
// NOT fmaf((float)nibble, scale, -8.0f * scale), one operation fewer: its one rounding is the rule's for every non-zero result, but the sign of a zero
// result is not - nibble 8 gives 8 scale + (-8 scale) = +0.0 where the rule's 0 * scale is -0.0 (scale is negative), and with scale = -0.0 it gives
// -0.0 + +0.0 = +0.0 for every nibble where the rule gives +0.0 below 8 and -0.0 from 8 on.  Rows are compared bit for bit, so the product it is.
__device__ __forceinline__ void kv4_deq8(f32x4v& a, f32x4v& b, uint32_t w, float s) {
    const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
    a = f32x4v{((float)(lo & 255u) - 8.0f) * s, ((float)(hi & 255u) - 8.0f) * s, ((float)((lo >> 8) & 255u) - 8.0f) * s, ((float)((hi >> 8) & 255u) - 8.0f) * s};
    b = f32x4v{((float)((lo >> 16) & 255u) - 8.0f) * s, ((float)((hi >> 16) & 255u) - 8.0f) * s, ((float)(lo >> 24) - 8.0f) * s, ((float)(hi >> 24) - 8.0f) * s};
}

// ... and where a lane's word lives: elements e .. e + 7 (e a multiple of 8) of the K (which = 0) or V (1) row of in-page position pin.  [layer][kv head]
// [hs / 32] is [layer][kv_dim / 32] - a head is a whole number of groups.  The group's first lane stores the scale.
__device__ __forceinline__ void kv4_store8(uint8_t* k_page, uint8_t* v_page, size_t nib_bytes, int which, int layer, int kv, int hs, int PL, int pin, int e, uint32_t w,
                                           float scale) {
    if (which == 0) {
        const size_t cell = ((size_t)layer * (kv >> 5) + (e >> 5)) * PL + pin;
        *reinterpret_cast<uint32_t*>(k_page + cell * 16 + ((e & 31) >> 1)) = w;
        if ((e & 31) == 0) reinterpret_cast<float*>(k_page + nib_bytes)[cell] = scale;
    } else {
        const int head = e / hs, d = e - head * hs;
        const size_t row = ((size_t)layer * (kv / hs) + head) * PL + pin;
        *reinterpret_cast<uint32_t*>(v_page + row * (hs >> 1) + (d >> 1)) = w;
        if ((e & 31) == 0) reinterpret_cast<float*>(v_page + nib_bytes)[row * (hs >> 5) + (d >> 5)] = scale;
    }
}

// One workgroup per row: q rotated in place, k rotated IN PLACE too (the attention launch reads it as the row's own key), then the rotated k row and the
// v row - 2 kv_dim consecutive floats of the qkv row - eight elements a lane, four lanes a group, a lane's eight nibbles one dword store
KV4_KERNEL __launch_bounds__(256) void kv4_scatter_kernel(float* qkv, uint8_t* k_pool, uint8_t* v_pool, const float* rope, const RowView rows, const KvqView pv,
                                                           int n_heads, int n_kv_heads, int hs, int layer) {
    const int r = blockIdx.x, pos = rows.pos[r], PL = 1 << pv.shift, pin = pos & (PL - 1);
    const size_t off = (size_t)pv.tab[(size_t)rows.off[r] * pv.per_slot + (pos >> pv.shift)] * pv.page_bytes;
    float* row = qkv + (size_t)r * (n_heads + 2 * n_kv_heads) * hs;
    const int half = hs / 2, att = n_heads * hs, kv = n_kv_heads * hs;
    for (int i = threadIdx.x; i < (n_heads + n_kv_heads) * half; i += blockDim.x) {
        const int hh = i / half, j = i - hh * half;
        const float2 cs = *reinterpret_cast<const float2*>(rope + ((size_t)pos * half + j) * 2);
        float* p = row + hh * hs;                         // (the k heads follow the q heads in the row)
        const float2 rq = rope_rotate(p[j], p[j + half], cs.x, cs.y);
        p[j] = rq.x; p[j + half] = rq.y;
    }
    __syncthreads();
    const float4* src = reinterpret_cast<const float4*>(row + att);
    const int kv8 = kv / 8;                               // a multiple of 4: whole clusters stay active together
    for (int i = threadIdx.x; i < 2 * kv8; i += blockDim.x) {
        const int which = i >= kv8, e = (i - which * kv8) * 8;
        float scale;
        const uint32_t w = kv4_quant8(src[2 * i], src[2 * i + 1], scale);
        kv4_store8(k_pool + off, v_pool + off, pv.q_bytes, which, layer, kv, hs, PL, pin, e, w, scale);
    }
}

// pv.q_bytes: nib_bytes, the nibbles of a page's K (or V) block
hipError_t launch_kv4_scatter(float* qkv, float* k_pool, float* v_pool, const float* rope, RowView rows, KvqView pv, int n_heads, int n_kv_heads, int hs,
                              int layer, int n_rows, hipStream_t s) {
    if (n_rows < 1 || n_rows > kRunRowsMax || !pv.tab || pv.shift < 6 || pv.per_slot < 1 || !pv.q_bytes || hs % 32) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv4_scatter_kernel, dim3(n_rows), dim3(256), 0, s, qkv, reinterpret_cast<uint8_t*>(k_pool), reinterpret_cast<uint8_t*>(v_pool), rope, rows, pv,
                       n_heads, n_kv_heads, hs, layer);
    return hipGetLastError();
}

// lmrs_batch_fork from the context's own cache: rows p0 .. of the f32 cache (K blocked [layer][kv_dim / 4][S][4], V [layer][S][kv_dim]) through the
// scatter's two device functions into in-page positions pin0 .. of ONE page; one workgroup per (row, layer)
KV4_KERNEL __launch_bounds__(256) void kv4_import_kernel(const float* k_src, const float* v_src, int S, int p0, uint8_t* k_page, uint8_t* v_page, size_t nib_bytes,
                                                          int kv, int hs, int PL, int pin0) {
    const int layer = blockIdx.y, p = p0 + blockIdx.x, pin = pin0 + blockIdx.x, kv8 = kv / 8;
    for (int i = threadIdx.x; i < 2 * kv8; i += blockDim.x) {
        const int which = i >= kv8, e = (i - which * kv8) * 8;
        float4 a, b;
        if (which) {
            const float4* v = reinterpret_cast<const float4*>(v_src + ((size_t)layer * S + p) * kv + e);
            a = v[0]; b = v[1];
        } else {
            const float* k = k_src + (((size_t)layer * (kv / 4) + (e >> 2)) * S + p) * 4;
            a = *reinterpret_cast<const float4*>(k); b = *reinterpret_cast<const float4*>(k + (size_t)S * 4);
        }
        float scale;
        const uint32_t w = kv4_quant8(a, b, scale);
        kv4_store8(k_page, v_page, nib_bytes, which, layer, kv, hs, PL, pin, e, w, scale);
    }
}
hipError_t launch_kv4_import(const float* k_src, const float* v_src, int seq_len, int p0, float* k_page, float* v_page, size_t nib_bytes, int n_layers, int kv, int hs,
                             int page_len, int pin0, int n_rows, hipStream_t s) {
    if (n_rows < 1 || pin0 < 0 || pin0 + n_rows > page_len || p0 < 0 || p0 + n_rows > seq_len || hs % 32 || kv % hs || !nib_bytes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv4_import_kernel, dim3(n_rows, n_layers), dim3(256), 0, s, k_src, v_src, seq_len, p0, reinterpret_cast<uint8_t*>(k_page),
                       reinterpret_cast<uint8_t*>(v_page), nib_bytes, kv, hs, page_len, pin0);
    return hipGetLastError();
}

// lmrs_op_kv4_round_trip: caller values through kv4_quant8 and kv4_deq8 themselves, eight a lane, nothing stored in between
KV4_KERNEL __launch_bounds__(256) void kv4_round_trip_kernel(const float* x, float* out, int n8) {
    const int i = blockIdx.x * 256 + threadIdx.x;         // n8 is a multiple of 4: a cluster is live or idle as a whole
    if (i >= n8) return;
    const float4* src = reinterpret_cast<const float4*>(x) + 2 * (size_t)i;
    float scale;
    const uint32_t w = kv4_quant8(src[0], src[1], scale);
    f32x4v a, b;
    kv4_deq8(a, b, w, scale);
    *reinterpret_cast<f32x4v*>(out + (size_t)i * 8) = a;
    *reinterpret_cast<f32x4v*>(out + (size_t)i * 8 + 4) = b;
}
hipError_t launch_kv4_round_trip(const float* x, float* out, size_t n, hipStream_t s) {
    if (n < 32 || n % 32 || n > ((size_t)1 << 30)) return hipErrorInvalidValue;
    const int n8 = (int)(n / 8);
    hipLaunchKernelGGL(kv4_round_trip_kernel, dim3((n8 + 255) / 256), dim3(256), 0, s, x, out, n8);
    return hipGetLastError();
}

// ---- scores.  One lane per key, as paged_score_chain; a batch is 32 dims of the lane's key - ONE 16-byte word and its scale - and the batches
// ping-pong as raw words: five registers in flight a batch.  The conversion lands in the eight f32x4v att_kuse consumes.
struct Kv4Key { const uint8_t* q; const float* s; };      // this lane's key inside ITS page: its first group's word and scale
struct Kv4Raw { i32x4v w; float s; };
__device__ __forceinline__ void kv4_kload(Kv4Raw& r, const Kv4Key k, int b, int PL) {
    r.w = *reinterpret_cast<const i32x4v*>(k.q + (size_t)b * PL * 16);
    r.s = k.s[(size_t)b * PL];
}
// the batch's 32 dims: read back - or, in the lane of the row's own position, taken from the f32 key (kown: the rotated k of the qkv row, in LDS)
__device__ __forceinline__ void kv4_kdeq(f32x4v (&kf)[8], const Kv4Raw& r, const float* kown, bool own) {
#pragma unroll
    for (int u = 0; u < 4; ++u) kv4_deq8(kf[2 * u], kf[2 * u + 1], (uint32_t)r.w[u], r.s);
    if (own) {
#pragma unroll
        for (int u = 0; u < 8; ++u) kf[u] = *reinterpret_cast<const f32x4v*>(kown + u * 4);
    }
}
template <int HS>
__device__ __forceinline__ float kv4_score_chain(Kv4Raw& ra, const Kv4Key k, const float* q, const float* kown, bool own, int PL) {
    constexpr int NB = HS / 32;
    Kv4Raw rb;
    f32x4v kf[8];
    float score = 0.0f;
    const float4* q4 = reinterpret_cast<const float4*>(q);
#pragma unroll
    for (int b = 0; b < NB; b += 2) {
        if (b + 1 < NB) kv4_kload(rb, k, b + 1, PL);
        kv4_kdeq(kf, ra, kown + b * 32, own);
        score = att_kuse<8>(score, kf, q4, b * 8);
        asm volatile("" : "+v"(score) : : "memory");
        if (b + 1 < NB) {
            if (b + 2 < NB) kv4_kload(ra, k, b + 2, PL);
            kv4_kdeq(kf, rb, kown + (b + 1) * 32, own);
            score = att_kuse<8>(score, kf, q4, (b + 1) * 8);
            asm volatile("" : "+v"(score) : : "memory");
        }
    }
    return score;
}

// ---- values.  A chunk is 64 rows of the kv head: 64 * HS / 16 pieces of 16 dims - 8 bytes of nibbles, so that every lane of the workgroup unpacks at
// every head size - piece f = tid + i * 256 in slot i of a lane (row f / (HS / 16)), its two words and its group's scale the prefetch buffer: three
// registers a piece where Q8 holds five.  Head-major rows: piece f is 8 f bytes into the chunk, a wave's 64 loads 512 consecutive bytes.  Rows past the
// chunk's last are clamped to it and meet the zero-padded weights, as in att_gload / att_tstore.
struct Kv4Val { i32x2v w; float s; };
template <int HS, int NP>
__device__ __forceinline__ void kv4_vload(Kv4Val (&rg)[NP], const uint8_t* vq, const float* vs, int pin0, int ct) {
    constexpr int HS16 = HS / 16;
    const int nf = ((ct + 15) & ~15) * HS16;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int f = (int)threadIdx.x + i * kBlock;
        if (f < nf) {
            int row = f / HS16;
            const int c16 = f - row * HS16;
            row = pin0 + (row < ct - 1 ? row : ct - 1);
            rg[i].w = *reinterpret_cast<const i32x2v*>(vq + (size_t)row * (HS / 2) + c16 * 8);
            rg[i].s = vs[(size_t)row * (HS / 32) + (c16 >> 1)];
        }
    }
}
// registers -> the LDS tile, each value read back and multiplied by its row's weight (att_tstore's multiply); the row of the pass's own position
// takes the f32 v (vown, in LDS) in the place of the read-back, in the lanes that hold that row
template <int HS, int NP>
__device__ __forceinline__ void kv4_tstore(const Kv4Val (&rg)[NP], float* tile, const float* rowscale, int t0, int ct, int pos, const float* vown) {
    constexpr int HS16 = HS / 16, RS = HS + 4;
    const int nf = ((ct + 15) & ~15) * HS16;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int f = (int)threadIdx.x + i * kBlock;
        if (f < nf) {
            const int row = f / HS16, c16 = f - row * HS16;
            const float sc = rowscale[row];
            f32x4v v[4];
            kv4_deq8(v[0], v[1], (uint32_t)rg[i].w[0], rg[i].s);
            kv4_deq8(v[2], v[3], (uint32_t)rg[i].w[1], rg[i].s);
            if (t0 + row == pos) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4v*>(vown + c16 * 16 + u * 4);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                f32x4v p;
                p.x = sc * v[u].x; p.y = sc * v[u].y; p.z = sc * v[u].z; p.w = sc * v[u].w;
                *reinterpret_cast<f32x4v*>(tile + row * RS + c16 * 16 + u * 4) = p;
            }
        }
    }
}

// paged_attention_body over Q4 pages: a.q the row's qkv row (q rotated, k rotated, v), the LDS layout attention_body's - its spare 2 HS floats behind q
// take the row's own key and value
template <int HS, bool GEMMA>
__device__ __forceinline__ void kv4_attention_body(const AttnArgs& a, const uint8_t* k_pool, const uint8_t* v_pool, const uint32_t* tab, const KvqView& pv, int h, int pos,
                                                   char* smem, uint64_t etab) {
    constexpr int RS = HS + 4, CH = 64, NP = (CH * (HS / 16) + kBlock - 1) / kBlock;
    static_assert(HS % 32 == 0, "a group of 32 never straddles a head");
    const int kv_mul = a.n_heads / a.n_kv_heads, kvh = h / kv_mul;
    const int att_dim = a.n_heads * HS, kv_dim = a.n_kv_heads * HS;
    const int T = pos + 1;
    const int tid = threadIdx.x;
    const int shift = pv.shift, PL = 1 << shift;
    float* q = reinterpret_cast<float*>(smem);
    float* kown = q + HS;
    float* vown = q + 2 * HS;
    float* red = q + 3 * HS;
    float* tile = red + 16;
    float* att = tile + (size_t)(CH + 32) * RS;
    const int nchunks = (T + CH - 1) / CH;
    const size_t head = (size_t)a.layer * a.n_kv_heads + kvh;
    const size_t kq_head = head * (HS / 32) * (size_t)PL * 16;                          // bytes into a page's K block
    const size_t ks_head = pv.q_bytes + head * (HS / 32) * (size_t)PL * 4;
    const size_t vq_head = head * (size_t)PL * (HS / 2);                                // ... its V block
    const size_t vs_head = pv.q_bytes + head * (size_t)PL * (HS / 32) * 4;
    auto key_of = [&](int t) __attribute__((always_inline)) {
        const uint8_t* page = k_pool + (size_t)tab[t >> shift] * pv.page_bytes;
        const int pin = t & (PL - 1);
        return Kv4Key{page + kq_head + (size_t)pin * 16, reinterpret_cast<const float*>(page + ks_head) + pin};
    };
    // CH divides page_len, so a chunk lies in ONE page - one table lookup a chunk
    auto v_load = [&](Kv4Val (&rg)[NP], int t0) __attribute__((always_inline)) {
        const uint8_t* page = v_pool + (size_t)tab[t0 >> shift] * pv.page_bytes;
        kv4_vload<HS, NP>(rg, page + vq_head, reinterpret_cast<const float*>(page + vs_head), t0 & (PL - 1), (T - t0) < CH ? (T - t0) : CH);
    };
    const int tc0 = tid < T ? tid : T - 1;            // lanes past the sequence repeat its last key (no predication)
    const Kv4Key kp0 = key_of(tc0);
    Kv4Raw ka;
    kv4_kload(ka, kp0, 0, PL);
    Kv4Val vreg[NP];
    v_load(vreg, 0);
    for (int j = tid; j < HS; j += kBlock) {
        q[j] = a.q[h * HS + j];
        kown[j] = a.q[att_dim + kvh * HS + j];
        vown[j] = a.q[att_dim + kv_dim + kvh * HS + j];
    }
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
    finish_score(kv4_score_chain<HS>(ka, kp0, q, kown, tc0 == pos, PL), tid);
    for (int t0 = kBlock; t0 < T; t0 += kBlock) {
        const int t = t0 + tid, tc = t < T ? t : T - 1;
        const Kv4Key kp = key_of(tc);
        Kv4Raw k0;
        kv4_kload(k0, kp, 0, PL);
        finish_score(kv4_score_chain<HS>(k0, kp, q, kown, tc == pos, PL), t);
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

    // ---- weighted sum of values: products into the tile, one lane per output dim adds them up sequentially over t; the next chunk's words are in
    // flight under the sums
    float o = 0.0f;
    for (int c = 0; c < nchunks; ++c) {
        const int t0 = c * CH, ct = (T - t0) < CH ? (T - t0) : CH;
        kv4_tstore<HS, NP>(vreg, tile, att + t0, t0, ct, pos, vown);
        lds_barrier();
        if (c + 1 < nchunks) v_load(vreg, t0 + CH);
        if (tid < HS) o = serial_sum16<RS, false>(o, tile + tid, ct);
        lds_barrier();
    }
    if (tid < HS) a.out[h * HS + tid] = o;
}

// one workgroup per (head, row) over a RowView, as paged_attn_kernel
template <int HS, bool GEMMA>
KV4_KERNEL __launch_bounds__(kBlock) void kv4_attn_kernel(const AttnArgs a0, const RowView rows, const KvqView pv) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AttnArgs a = a0;
    const int r = blockIdx.y, h = blockIdx.x, att = a.n_heads * HS, kv = a.n_kv_heads * HS;
    a.q = a0.q + (size_t)r * (att + 2 * kv); a.out = a0.out + (size_t)r * att; a.dbg = nullptr;
    const uint64_t etab = exp2f_tab_lane();
    kv4_attention_body<HS, GEMMA>(a, reinterpret_cast<const uint8_t*>(a0.k_cache), reinterpret_cast<const uint8_t*>(a0.v_cache), pv.tab + (size_t)rows.off[r] * pv.per_slot, pv, h,
                                  rows.pos[r], smem, etab);
}

hipError_t launch_kv4_attention(const AttnArgs& a0, RowView rows, KvqView pv, int n_rows, int max_T, hipStream_t s) {
    AttnArgs a = a0;
    a.chunk = 64;                                                          // the kernels' CH; 64 divides every page_len
    if (n_rows < 1 || n_rows > kRunRowsMax || max_T < 1 || max_T > a.seq_len) return hipErrorInvalidValue;
    if (!pv.tab || pv.shift < 6 || pv.per_slot < 1 || !pv.q_bytes) return hipErrorInvalidValue;
    const size_t smem = attention_smem(a.head_size, a.chunk, max_T);
#define A4(HS_, G_)                                                                                                                   \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(kv4_attn_kernel<HS_, G_>));                                                       \
        hipLaunchKernelGGL((kv4_attn_kernel<HS_, G_>), dim3(a.n_heads, n_rows), dim3(kBlock), smem, s, a, rows, pv);                   \
        return hipGetLastError();                                                                                                     \
    }
    if (a.gemma) { if (a.head_size == 256) A4(256, true) return hipErrorInvalidValue; }
    switch (a.head_size) { case 64: A4(64, false) case 96: A4(96, false) case 128: A4(128, false) default: return hipErrorInvalidValue; }
#undef A4
}

// ------------------------------------------------------------------------------------------------
// BLOCK attention over Q4 pages: launch_kvq_attention_block's three launches (lmrs_kvq.inc) with the two readers of the cache reading nibbles.  The
// scatter (launch_kv4_scatter over the chunk's rows) has ended: q and k of every qkv row are rotated, every key and value row of the chunk is in the slot's
// pages, quantised.  The contract is the table pass's at the top of this file: a query at position p takes keys and values 0 .. p-1 as kv4_deq8 reads
// them back and its OWN key and value in f32 from its qkv row; keys behind p inside the 64-query block are read back and meet weight 0.0.  The diagonal
// is the Q8 block kernels' (block_kvq_own_dot over S[p] in the wave that owns key p, block_kvq_tile_compute_own in the tiles that hold positions of the
// query block), and everything behind the two loaders - the four score chains, the division by sqrtf(HS), the cap and window term, the softmax launch,
// the tiles two ahead - is the f32 block kernels', so the output carries kv4_attn_kernel's bits whatever the chunking.
// The loaders are this layout's own:
//   keys    a chunk of NK keys is NK * HS / 32 words of 16 bytes, fewer than the workgroup has threads at HS 64 and in Gemma's 32-key form.  A thread's
//           share of the chunk is NK * HS / 2 / NT bytes - 8 / 12 / 16 at HS 64 / 96 / 128, 8 and 32 in Gemma's two forms - and its PIECE the largest of
//           16, 8 or 4 bytes that divides the share: one half word, three quarter words, one word, one half word, two words.  Pieces are numbered within a
//           word first, then key by key, then group by group, so consecutive lanes read consecutive bytes of a group's NK * 16 - every thread loads and
//           converts, every line is read whole.  A piece and the scale of its group wait in registers under the query rows' staging (at most ten a
//           thread) and go through kv4_deq8 into the f32 tile att_kread consumes.
//   values  V is head-major: a tile row's slice of SW dims is SW / 2 consecutive bytes, HS / 2 from the next row's.  One 16-dim piece a thread - two words
//           and the scale of ITS group of 32 (a 48-dim slice of a 96-wide head starts in the middle of a group), three registers where Q8 holds five -
//           kept two tiles ahead as raw words (Kv4Val) and read back on the way into LDS.  The weight half of the tile is the f32 kernels'.
// ------------------------------------------------------------------------------------------------
template <int PB> struct Kv4Piece { uint32_t w[PB / 4]; float s; };
template <int HS, int RS, int NK, int NT>
__device__ __forceinline__ void block_kv4_stage(float* qt, float* kt, const float* __restrict__ qrows, int qs, const uint8_t* __restrict__ k_pool, const KvqPages pg,
                                                int n_kv_heads, int h, int kvh, int qb, int cb, int bT, int n_tok) {
    constexpr int HS4 = HS / 4, SHARE = NK * HS / 2 / NT, PB = SHARE % 16 == 0 ? 16 : SHARE % 8 == 0 ? 8 : 4, NP = SHARE / PB, SUB = 16 / PB;
    static_assert(HS % 32 == 0 && NP >= 1 && NP * NT * PB == NK * HS / 2 && (NK & (NK - 1)) == 0, "every thread the same number of whole pieces");
    const int tid = threadIdx.x, PL = 1 << pg.shift;
    const int kc = cb < bT ? cb : bT - 1;                                     // the chunk's first key, clamped: its page holds every clamped key of the chunk
    const uint8_t* page = k_pool + (size_t)pg.tab[kc >> pg.shift] * pg.page_bytes;
    const size_t head = ((size_t)pg.layer * n_kv_heads + kvh) * (HS / 32) * (size_t)PL;
    const uint8_t* kq = page + head * 16;                                     // [HS/32][page_len][16]
    const float* ks = reinterpret_cast<const float*>(page + pg.q_bytes) + head;          // [HS/32][page_len]
    Kv4Piece<PB> raw[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int f = tid + i * NT, sub = f % SUB, kl = (f / SUB) % NK, g = f / (SUB * NK);
        const int pin = (cb + kl < bT ? cb + kl : bT - 1) & (PL - 1);
        const uint8_t* src = kq + ((size_t)g * PL + pin) * 16 + sub * PB;
        if constexpr (PB == 16) {
            const i32x4v w = *reinterpret_cast<const i32x4v*>(src);
#pragma unroll
            for (int u = 0; u < 4; ++u) raw[i].w[u] = (uint32_t)w[u];
        } else if constexpr (PB == 8) {
            const i32x2v w = *reinterpret_cast<const i32x2v*>(src);
            raw[i].w[0] = (uint32_t)w[0]; raw[i].w[1] = (uint32_t)w[1];
        } else raw[i].w[0] = *reinterpret_cast<const uint32_t*>(src);
        raw[i].s = ks[(size_t)g * PL + pin];
    }
    for (int f = tid; f < 64 * HS4; f += NT) {
        const int r = f / HS4, c4 = f - r * HS4;
        int qi = qb * kAttQB + r; qi = qi < n_tok ? qi : n_tok - 1;
        *reinterpret_cast<float4*>(qt + r * RS + c4 * 4) = *reinterpret_cast<const float4*>(qrows + (size_t)qi * qs + h * HS + c4 * 4);
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int f = tid + i * NT, sub = f % SUB, kl = (f / SUB) % NK, g = f / (SUB * NK);
        float* dst = kt + kl * RS + g * 32 + sub * (2 * PB);                  // a byte is two dims
#pragma unroll
        for (int u = 0; u < PB / 4; ++u) {
            f32x4v a, b;
            kv4_deq8(a, b, raw[i].w[u], raw[i].s);
            *reinterpret_cast<f32x4v*>(dst + u * 8) = a;
            *reinterpret_cast<f32x4v*>(dst + u * 8 + 4) = b;
        }
    }
}
template <int HS>
KV4_KERNEL __launch_bounds__(256) void block_kv4_scores_kernel(const float* __restrict__ qrows, int qs, const uint8_t* __restrict__ k_pool, const KvqPages pg,
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
    block_kv4_stage<HS, RS, 64, 256>(qt, kt, qrows, qs, k_pool, pg, n_kv_heads, h, kvh, qb, cb, b.T, n_tok);
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
    // the diagonal: this wave owns the lane's own position (p <= T - 1, so p < c0 + 16 is p < c0 + nk) - the f32 key of its qkv row, over S[p]
    if (b.p >= c0 && b.p < c0 + 16) {
        const float* kown = qrows + (size_t)b.i * qs + n_heads * HS + kvh * HS;
        S[(size_t)b.p * kAttQB] = block_kvq_own_dot<HS4>(0.0f, q, kown) / sqrt_hs;
    }
}
// Gemma-2's 256-wide heads: NK keys a workgroup of NT threads, two passes of 128 dims over one chain; the diagonal's key comes from memory
template <int HS, int NK, int NT>
KV4_KERNEL __launch_bounds__(NT) void block_kv4_scores_wide_kernel(const float* __restrict__ qrows, int qs, const uint8_t* __restrict__ k_pool, const KvqPages pg,
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
    block_kv4_stage<HS, RS, NK, NT>(qt, kt, qrows, qs, k_pool, pg, n_kv_heads, h, kvh, qb, cb, b.T, n_tok);
    __syncthreads();
    const int c0 = cb + wave * KW;
    if (c0 >= b.T) return;
    const int nk = b.T - c0 < KW ? b.T - c0 : KW;
    const float* kv = kt + wave * KW * RS;
    const bool mine = b.p >= c0 && b.p < c0 + KW;                // this wave owns the lane's own position
    const float* kown = qrows + (size_t)b.i * qs + n_heads * HS + kvh * HS;
    float own = 0.0f;
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
        if (mine) own = block_kvq_own_dot<HP4>(own, q, kown + pass * HP);       // the pass's 128 dims of the one chain
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
    if (mine) S[(size_t)b.p * kAttQB] = gemma_cap_window(own / sqrt_hs, wpos, b.p);
}

// A tile's loads: the weights as in the f32 kernels; of the value tile one 16-dim piece a thread (64 * SW / 16 <= NT) - its two raw words and the scale of its
// group of 32.  vq: bytes into a page's V block of this head's rows at the slice's first dim d0 (of the head); vs: floats into its scales of this head's rows.
// Threads past the tile repeat its last piece (no load under a branch) and store nothing.
template <int HS, int NT, int SW, int NS>
__device__ __forceinline__ void block_kv4_tile_load(f32x4v (&rw)[NS], Kv4Val& rv, const float* Sb, const uint8_t* v_pool, size_t vq, size_t vs, int d0, const KvqPages pg,
                                                    int t, int T) {
    constexpr int S16 = SW / 16, NPC = 64 * S16;
    static_assert(SW % 16 == 0 && NPC <= NT, "a piece a thread");
    const int tid = threadIdx.x, k0 = t * 64, PL = 1 << pg.shift;
    const int kc = k0 < T ? k0 : T - 1;                                       // the tile's first key, clamped (a prefetch past the end: the last key's page)
    const uint8_t* vb = v_pool + (size_t)pg.tab[kc >> pg.shift] * pg.page_bytes;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int f = tid + j * NT, kl = f >> 4, c4 = f & 15;
        const int key = k0 + kl < T ? k0 + kl : T - 1;
        const f32x4v w4 = *reinterpret_cast<const f32x4v*>(Sb + (size_t)key * kAttQB + c4 * 4);
        rw[j] = k0 + kl < T ? w4 : f32x4v{0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int f = tid < NPC ? tid : NPC - 1, kl = f / S16, c16 = f - kl * S16;
    const int pin = (k0 + kl < T ? k0 + kl : T - 1) & (PL - 1);
    rv.w = *reinterpret_cast<const i32x2v*>(vb + vq + (size_t)pin * (HS / 2) + c16 * 8);
    rv.s = reinterpret_cast<const float*>(vb + pg.q_bytes)[vs + (size_t)pin * (HS / 32) + ((d0 + c16 * 16) >> 5)];
}
// att_tile_store with the read-back in it, on the way into the [64][SW] f32 tile att_tile_compute reads
template <int NT, int SW, int NS>
__device__ __forceinline__ void block_kv4_tile_store(const f32x4v (&rw)[NS], const Kv4Val& rv, float* dst) {
    constexpr int S16 = SW / 16;
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < NS; ++j) { const int f = tid + j * NT; *reinterpret_cast<f32x4v*>(dst + f * 4) = rw[j]; }
    if (tid < 64 * S16) {
        f32x4v v[4];
        kv4_deq8(v[0], v[1], (uint32_t)rv.w[0], rv.s);
        kv4_deq8(v[2], v[3], (uint32_t)rv.w[1], rv.s);
#pragma unroll
        for (int u = 0; u < 4; ++u) *reinterpret_cast<f32x4v*>(dst + 64 * 64 + tid * 16 + u * 4) = v[u];           // piece tid: row tid / S16, dims (tid % S16) * 16 ..
    }
}
template <int HS, int NW, int DW>
KV4_KERNEL __launch_bounds__(NW * 64) void block_kv4_values_kernel(const float* __restrict__ qrows, int qs, const uint8_t* __restrict__ v_pool, const KvqPages pg,
                                                                    const float* __restrict__ scratch, float* __restrict__ out, int n_heads, int n_kv_heads,
                                                                    int pos0, int n_tok, int Tmax) {
    constexpr int NT = NW * 64, SW = NW * DW, NS = 64 * 16 / NT;
    static_assert(HS % SW == 0 && HS % 32 == 0 && DW % 4 == 0 && (64 * 16) % NT == 0, "slice geometry");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sm = reinterpret_cast<float*>(smem_raw);
    constexpr int TILE = 64 * 64 + 64 * SW;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = blockIdx.x, sl = blockIdx.z;
    const int qb = (sl & 1) ? (int)blockIdx.y : (int)(gridDim.y - 1 - blockIdx.y);
    const AttBlock b = att_block(qb, lane, pos0, n_tok);
    const int T = b.T, n_tiles = (T + 63) / 64;
    const int kv_mul = n_heads / n_kv_heads, kvh = h / kv_mul, kv_dim = n_kv_heads * HS, att = n_heads * HS;
    const float* Sb = scratch + ((size_t)h * gridDim.y + qb) * (size_t)Tmax * kAttQB;
    const int d0 = sl * SW;                                                   // the slice's first dim of the head
    const size_t rows = ((size_t)pg.layer * n_kv_heads + kvh) << pg.shift;    // head-major: this head's page_len rows
    const size_t vq = rows * (HS / 2) + d0 / 2, vs = rows * (HS / 32);
    const int t_own = (pos0 + qb * kAttQB) >> 6;                              // the first tile with a position of this query block: it and the next are the last two
    float own[DW];
    {
        const float* vown = qrows + (size_t)b.i * qs + att + kv_dim + kvh * HS + d0 + wave * DW;
#pragma unroll
        for (int g = 0; g < DW / 4; ++g) {
            const float4 v4 = *reinterpret_cast<const float4*>(vown + g * 4);
            own[g * 4] = v4.x; own[g * 4 + 1] = v4.y; own[g * 4 + 2] = v4.z; own[g * 4 + 3] = v4.w;
        }
    }
    f32x4v rwa[NS], rwb[NS];
    Kv4Val rva, rvb;
    float acc[DW];
#pragma unroll
    for (int d = 0; d < DW; ++d) acc[d] = 0.0f;
    auto compute = [&](const float* cur, int t) __attribute__((always_inline)) {
        if (t >= t_own) block_kvq_tile_compute_own<DW, SW>(acc, cur, lane, wave, T - t * 64, b.p - t * 64, own);
        else att_tile_compute<HS, DW, SW>(acc, cur, lane, wave, T - t * 64);
    };
    block_kv4_tile_load<HS, NT, SW, NS>(rwa, rva, Sb, v_pool, vq, vs, d0, pg, 0, T);
    block_kv4_tile_store<NT, SW, NS>(rwa, rva, sm);
    block_kv4_tile_load<HS, NT, SW, NS>(rwa, rva, Sb, v_pool, vq, vs, d0, pg, 1, T);
    block_kv4_tile_load<HS, NT, SW, NS>(rwb, rvb, Sb, v_pool, vq, vs, d0, pg, 2, T);
    lds_barrier();
    for (int t = 0; t < n_tiles; t += 2) {
        compute(sm, t);
        if (t + 1 < n_tiles) block_kv4_tile_store<NT, SW, NS>(rwa, rva, sm + TILE);
        block_kv4_tile_load<HS, NT, SW, NS>(rwa, rva, Sb, v_pool, vq, vs, d0, pg, t + 3, T);
        lds_barrier();
        if (t + 1 < n_tiles) {
            compute(sm + TILE, t + 1);
            if (t + 2 < n_tiles) block_kv4_tile_store<NT, SW, NS>(rwb, rvb, sm);
            block_kv4_tile_load<HS, NT, SW, NS>(rwb, rvb, Sb, v_pool, vq, vs, d0, pg, t + 4, T);
            lds_barrier();
        }
    }
    if (b.live) {
        float* ob = out + (size_t)b.i * att + h * HS + d0 + wave * DW;
#pragma unroll
        for (int g = 0; g < DW / 4; ++g) *reinterpret_cast<float4*>(ob + g * 4) = make_float4(acc[g * 4], acc[g * 4 + 1], acc[g * 4 + 2], acc[g * 4 + 3]);
    }
}

// launch_kvq_attention_block's choices and refusals over Q4 pages.  a.q: the qkv block as launch_kv4_scatter left it (q and k rotated; row stride
// att + 2 kv) - the score and the value launch read the rows' own keys and values from it; a.k_cache / a.v_cache: the pool's K and V block of page 0;
// pv.q_bytes: nib_bytes
hipError_t launch_kv4_attention_block(const AttnArgs& a, KvqView pv, unsigned table_row, int pos0, int n_tok, float* scratch, int lds_keys, bool long_forms, hipStream_t s) {
    const int T = pos0 + n_tok, nqb = (n_tok + kAttQB - 1) / kAttQB, nch = (T + 63) / 64;
    if (!pv.tab || pv.shift < 6 || pv.per_slot < 1 || !pv.q_bytes || n_tok < 1 || pos0 < 0 || T > a.seq_len || ((T - 1) >> pv.shift) >= pv.per_slot) return hipErrorInvalidValue;
    const int qs = (a.n_heads + 2 * a.n_kv_heads) * a.head_size;
    const KvqPages pg{pv.tab + (size_t)table_row * pv.per_slot, pv.shift, pv.page_bytes, pv.q_bytes, a.layer};
    const uint8_t* k_pool = reinterpret_cast<const uint8_t*>(a.k_cache);
    const uint8_t* v_pool = reinterpret_cast<const uint8_t*>(a.v_cache);
    const bool in_lds = T <= lds_keys;
    const size_t sm = (kAttSW * 64 + kAttSQ + (in_lds ? (size_t)(T + 48) * kAttSQ : 0)) * sizeof(float);
    allow_big_lds(reinterpret_cast<const void*>(att_softmax_kernel<true>));
    auto softmax = [&]() {
        if (in_lds) hipLaunchKernelGGL(att_softmax_kernel<true>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);
        else hipLaunchKernelGGL(att_softmax_kernel<false>, dim3(a.n_heads, nqb, kAttQB / kAttSQ), dim3(kAttSW * 64), sm, s, pos0, n_tok, scratch, T);
    };
#define V4(HS_, NW_, DW_)                                                                                                             \
    {                                                                                                                                 \
        allow_big_lds(reinterpret_cast<const void*>(block_kv4_values_kernel<HS_, NW_, DW_>));                                         \
        hipLaunchKernelGGL((block_kv4_values_kernel<HS_, NW_, DW_>), dim3(a.n_heads, nqb, HS_ / (NW_ * DW_)), dim3(NW_ * 64), 2 * (64 * 64 + 64 * NW_ * DW_) * sizeof(float), s, \
                           (const float*)a.q, qs, v_pool, pg, (const float*)scratch, a.out, a.n_heads, a.n_kv_heads, pos0, n_tok, T); \
        return hipGetLastError();                                                                                                     \
    }
#define B4(HS_, NW_, DW_)                                                                                                             \
    {                                                                                                                                 \
        hipLaunchKernelGGL((block_kv4_scores_kernel<HS_>), dim3(a.n_heads, nch, nqb), dim3(256), 0, s, (const float*)a.q, qs, k_pool, pg, scratch,        \
                           a.n_heads, a.n_kv_heads, pos0, n_tok, T);                                                                  \
        softmax();                                                                                                                    \
        V4(HS_, NW_, DW_)                                                                                                             \
    }
    if (a.gemma) {
        if (a.head_size != 256) return hipErrorInvalidValue;
        int live64 = 0;
        for (int qb = 0; qb < nqb; ++qb) { const int last = qb * kAttQB + kAttQB - 1 < n_tok - 1 ? qb * kAttQB + kAttQB - 1 : n_tok - 1; live64 += (pos0 + last + 1 + 63) / 64; }
        live64 *= a.n_heads;
        if (live64 < 512 && !long_forms) {
            constexpr size_t smem32 = (size_t)(64 + 32) * (256 + 4) * sizeof(float);
            allow_big_lds(reinterpret_cast<const void*>(block_kv4_scores_wide_kernel<256, 32, 512>));
            hipLaunchKernelGGL((block_kv4_scores_wide_kernel<256, 32, 512>), dim3(a.n_heads, (T + 31) / 32, nqb), dim3(512), smem32, s, (const float*)a.q, qs, k_pool, pg,
                               scratch, a.st, a.n_heads, a.n_kv_heads, pos0, n_tok, T);
        } else {
            constexpr size_t wide_smem = (size_t)2 * 64 * (256 + 4) * sizeof(float);
            allow_big_lds(reinterpret_cast<const void*>(block_kv4_scores_wide_kernel<256, 64, 256>));
            hipLaunchKernelGGL((block_kv4_scores_wide_kernel<256, 64, 256>), dim3(a.n_heads, nch, nqb), dim3(256), wide_smem, s, (const float*)a.q, qs, k_pool, pg,
                               scratch, a.st, a.n_heads, a.n_kv_heads, pos0, n_tok, T);
        }
        softmax();
        if (a.n_heads * nqb * 4 < 256 && !long_forms) V4(256, 8, 4)
        V4(256, 8, 8)
    }
    switch (a.head_size) { case 64: B4(64, 8, 4) case 96: B4(96, 4, 12) case 128: B4(128, 8, 8) default: return hipErrorInvalidValue; }
#undef B4
#undef V4
}
#undef KV4_KERNEL
