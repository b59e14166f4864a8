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
// kv_mul query heads - was not built or measured.
// Out of scope: block attention over Q4 pages (every prompt chunk takes this table pass), Q4 for contiguous and wide batches or the context's own
// cache, mixed K / V formats.
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
#undef KV4_KERNEL
