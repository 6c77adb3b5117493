// vlmc_rope: the rotary position embedding of a LLaMA attention (modeling_llama.py:126-140, `apply_rotary_pos_emb`) for q AND k in
// one launch.
//
// The reference gathers cos / sin rows by `position_ids` (two `repeat`s and two `torch.gather`s), builds `rotate_half(x)` (two slices,
// a negation, a `cat`) and forms `(x * cos) + (rotate_half(x) * sin)` -- for q and for k: ~16 elementwise / gather / cat launches and
// ~10 passes over [B, H, T, d] tensors per layer and forward.  Every tensor op rounds to the 16-bit dtype, so the kernel rounds in the
// same three places:  wd( wd(x * cos) + wd(rot(x) * sin) ), products and sum in fp32 (torch's opmath), the negation inside rot exact.
// One lane owns 8 consecutive d of one (batch, token, head) row of q and of k: 16-byte loads of the row, its partner half and the two
// table rows, 16-byte stores.  HBM-bound: q and k are read once (the partner half comes from the same cache lines) and written once.
// Rows behind a sample's length (q_len: a padded group of ragged samples) are not read and are written as zeros; a position outside
// the table is never read: the row is written as zeros and the caller's status word is set (vlmc_rope_status reports it).
#include "common.hpp"
#include "mfma.hpp"
#include "vec_access.hpp"

namespace vlmc {

struct RopeArgs {
    const uint16_t *q, *k;
    uint16_t *qo, *ko;
    const uint16_t *cos, *sin;
    const int64_t *pos;
    const int32_t *qlen;
    int32_t *status;
    int64_t sq_b, sq_h, sq_t, sk_b, sk_h, sk_t, so_b, so_h, so_t, ld, sp_b, sp_t, positions, total;   // elements; the d strides are 1
    int H, T, d;
};

// 8 elements of a row from element e on
__device__ __forceinline__ void rope_load8(const uint16_t *p, uint16_t (&e)[8]) {
    const u32x4_t v = load16_a2(p);
    __builtin_memcpy(e, &v, 16);
}

template <typename T> __device__ __forceinline__ uint16_t rope_one(uint16_t x, float rot, uint16_t c, uint16_t s) {
    float a = ieee_mul(to_f32<T>(x), to_f32<T>(c));
    asm volatile("" : "+v"(a));                                              // (a product of its own, rounded like `x * cos`)
    float b = ieee_mul(rot, to_f32<T>(s));
    asm volatile("" : "+v"(b));                                              // (.. like `rotate_half(x) * sin`)
    float r = ieee_add(to_f32<T>(from_f32<T>(a)), to_f32<T>(from_f32<T>(b)));
    asm volatile("" : "+v"(r));
    return from_f32<T>(r);
}

template <typename T> __global__ __launch_bounds__(256) void rope_kernel(const RopeArgs a) {
    const int cpr = a.d >> 3, half = a.d >> 1;                                // chunks of 8 per row
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < a.total; i += int64_t(gridDim.x) * 256) {
        const int ch = int(i % cpr);
        int64_t r = i / cpr;
        const int h = int(r % a.H);
        r /= a.H;
        const int t = int(r % a.T);
        const int64_t b = r / a.T;
        const int e0 = ch * 8;
        uint16_t *qo = a.qo + b * a.so_b + int64_t(h) * a.so_h + int64_t(t) * a.so_t + e0;
        uint16_t *ko = a.ko + b * a.so_b + int64_t(h) * a.so_h + int64_t(t) * a.so_t + e0;
        bool live = a.qlen == nullptr || t < a.qlen[b];
        int64_t p = 0;
        if (live) {
            p = a.pos[b * a.sp_b + int64_t(t) * a.sp_t];
            if (p < 0 || p >= a.positions) {                                  // never read: reported through the status word
                live = false;
                if (a.status != nullptr) atomicOr(reinterpret_cast<int *>(a.status), 1);
            }
        }
        uint16_t oq[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ok[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) {
            const uint16_t *qr = a.q + b * a.sq_b + int64_t(h) * a.sq_h + int64_t(t) * a.sq_t;
            const uint16_t *kr = a.k + b * a.sk_b + int64_t(h) * a.sk_h + int64_t(t) * a.sk_t;
            uint16_t xq[8], xk[8], pq[8], pk[8], c[8], s[8];
            rope_load8(qr + e0, xq);
            rope_load8(kr + e0, xk);
            rope_load8(a.cos + p * a.ld + e0, c);
            rope_load8(a.sin + p * a.ld + e0, s);
            // rotate_half(x)[j] = -x[j + d / 2] in the first half, x[j - d / 2] in the second
            if ((half & 7) == 0) {
                const int pe = e0 < half ? e0 + half : e0 - half;
                rope_load8(qr + pe, pq);
                rope_load8(kr + pe, pk);
            } else {                                                          // (d / 2 not a multiple of 8: a chunk's partners straddle two)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int pe = e0 + j < half ? e0 + j + half : e0 + j - half;
                    pq[j] = qr[pe];
                    pk[j] = kr[pe];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool neg = e0 + j < half;
                const float rq = to_f32<T>(pq[j]), rk = to_f32<T>(pk[j]);
                oq[j] = rope_one<T>(xq[j], neg ? -rq : rq, c[j], s[j]);
                ok[j] = rope_one<T>(xk[j], neg ? -rk : rk, c[j], s[j]);
            }
        }
        u32x4_t v;
        __builtin_memcpy(&v, oq, 16);
        store16_a2(qo, v);
        __builtin_memcpy(&v, ok, 16);
        store16_a2(ko, v);
    }
}

}  // namespace vlmc

using namespace vlmc;

extern "C" int vlmc_rope(const void *q, const void *k, void *q_out, void *k_out, int dtype, int64_t batch, int64_t heads, int64_t T,
                         int64_t head_dim, const int64_t *q_strides, const int64_t *k_strides, const int64_t *out_strides,
                         const void *cos, const void *sin, int64_t positions, int64_t table_ld, const int64_t *position_ids,
                         int64_t pos_stride_b, int64_t pos_stride_t, const int32_t *q_len, int32_t *status, void *stream) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "vlmc_rope: dtype must be VLMC_F16 or VLMC_BF16");
    VLMC_REQUIRE(q && k && q_out && k_out && cos && sin && position_ids && q_strides && k_strides && out_strides, "vlmc_rope: null pointer");
    VLMC_REQUIRE(batch > 0 && heads > 0 && T > 0, "vlmc_rope: empty problem");
    VLMC_REQUIRE(head_dim > 0 && head_dim <= 128 && head_dim % 8 == 0, "vlmc_rope: head_dim must be a multiple of 8, at most 128 (got %lld)",
                 (long long)head_dim);
    VLMC_REQUIRE(positions > 0 && table_ld >= head_dim, "vlmc_rope: the cos / sin tables need at least one row of head_dim entries");
    VLMC_REQUIRE(heads < (int64_t(1) << 20) && T < (int64_t(1) << 24) && batch < (int64_t(1) << 31), "vlmc_rope: shape too large");
    VLMC_REQUIRE(pos_stride_b >= 0 && pos_stride_t >= 0, "vlmc_rope: negative stride");
    for (int i = 0; i < 3; ++i)
        VLMC_REQUIRE(q_strides[i] >= 0 && k_strides[i] >= 0 && out_strides[i] > 0, "vlmc_rope: negative input stride or non-positive output stride");
    VLMC_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(q_out) |
                   reinterpret_cast<uintptr_t>(k_out) | reinterpret_cast<uintptr_t>(cos) | reinterpret_cast<uintptr_t>(sin)) & 1u) == 0,
                 "vlmc_rope: pointers must be 2-byte aligned");
    VLMC_REQUIRE(q_out != q && q_out != k && k_out != q && k_out != k && q_out != k_out, "vlmc_rope: the outputs must not alias the inputs");
    RopeArgs a{};
    a.q = static_cast<const uint16_t *>(q), a.k = static_cast<const uint16_t *>(k);
    a.qo = static_cast<uint16_t *>(q_out), a.ko = static_cast<uint16_t *>(k_out);
    a.cos = static_cast<const uint16_t *>(cos), a.sin = static_cast<const uint16_t *>(sin);
    a.pos = position_ids, a.qlen = q_len, a.status = status;
    a.sq_b = q_strides[0], a.sq_h = q_strides[1], a.sq_t = q_strides[2];
    a.sk_b = k_strides[0], a.sk_h = k_strides[1], a.sk_t = k_strides[2];
    a.so_b = out_strides[0], a.so_h = out_strides[1], a.so_t = out_strides[2];
    a.ld = table_ld, a.sp_b = pos_stride_b, a.sp_t = pos_stride_t, a.positions = positions;
    a.H = int(heads), a.T = int(T), a.d = int(head_dim);
    a.total = batch * T * heads * (head_dim / 8);
    int64_t blocks = (a.total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    const dim3 grid{unsigned(blocks)}, block{256};
    hipStream_t s = as_stream(stream);
    if (dtype == VLMC_F16) VLMC_LAUNCH_TIMED((rope_kernel<f16_t>), grid, block, s, a);
    else VLMC_LAUNCH_TIMED((rope_kernel<bf16_t>), grid, block, s, a);
    VLMC_HIP_CHECK_LAUNCH("vlmc_rope");
    return VLMC_OK;
}

extern "C" int vlmc_rope_status(const int32_t *status, void *stream) {
    VLMC_REQUIRE(status != nullptr, "vlmc_rope_status: null pointer");
    int32_t host = 0;
    hipStream_t s = as_stream(stream);
    if (hipMemcpyAsync(&host, status, sizeof(host), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
        set_error("vlmc_rope_status: cannot read the status word: %s", hipGetErrorString(hipGetLastError()));
        return VLMC_EHIP;
    }
    VLMC_REQUIRE(host == 0, "vlmc_rope: a position outside the cos / sin table (its rows were written as zeros, nothing was read)");
    return VLMC_OK;
}
