// A linear whose weight stays in the packed 2:4 format of pack24.hip or the packed 4:8 format of pack48.hip (both: values
// [N, K / 2] + meta [N, K / 8], 9 / 16 of the dense bytes), for the few rows of X a generation step brings (rows = batch x beams):
// there a linear costs the bytes of its weight.
//
//   Y[m][n] = wd(sum_k X[m][k] * W24[n][k] + bias[n])        W24 = unpack_24(values, meta)   (or unpack_48: W48)
//
// BIT FOR BIT what vlmc_linear_fwd gives on the unpacked weight, because an output element is accumulated exactly as in
// gemm_nt.hip: W rows are the A operand and X rows the B operand of v_mfma_f32_16x16x32_{f16,bf16}, a lane holds row lane & 15 and
// k = 8 * (lane >> 4) + j, ONE accumulator per element takes the K-steps of 32 in ascending order (missing chunks of the last
// step are zeros in both operands), the bias is added in fp32 after the last step, one rounding.  The pruned positions are real
// zeros in the A fragment and are multiplied like any other weight: an inf in X at a pruned column gives the NaN the dense
// layer gives.
//
// A lane's eight k of a K-step are one pack chunk -- 8 bytes of values and one byte of meta -- so the A fragment is expanded
// lane-locally in registers and W never touches LDS (what differs between the two formats is this expansion alone: Expand24 /
// Expand48 below); the B fragment is 16 contiguous bytes of a row of X (L2-resident: every
// workgroup reads all of X).  A workgroup owns 16 output features over all of K and keeps ceil(M / 16) accumulator tiles, so
// the packed weight is read from memory once whatever M is.
//
// One dependent MFMA chain per tile would leave one wave's loads in flight per 16 features.  The chain is therefore CARRIED
// round the workgroup's sixteen waves: K is cut into batches of D steps, batch b belongs to wave b % 16, and a wave starts its
// batch from the accumulators the previous batch's wave left in LDS (a turn counter in LDS orders them).  The moment a wave has
// handed on it issues the loads of its next batch, which are in flight while the other fifteen take their turns; the A
// fragments are expanded before the wave waits for its turn.  Same MFMAs, same order, same accumulator values as one chain:
// the same bits.
//
// M > vlmc_linear_fwd_24_max_rows() (prefill, the vision tower): compute-bound, so the entry point unpacks into the caller's
// workspace (unpack24_kernel / unpack48_kernel) and runs the dense launch -- the same bits by construction.  The entry points
// vlmc_linear_fwd_24_tiled / _48_tiled take any M without a workspace: the tiled GEMM of gemm_nt.hip with the weight operand packed
// (expanded between the global load and the LDS store), again the same bits; vlmc_linear_fwd_bm_tiled does the same for the bitmap format.
//
// The third format is the bitmap format of packbm.hip (ANY mask: values [nnz + 16], meta [N, K / 8], offs [N, ceil(K / 32)],
// rowptr [N + 1]), entry point vlmc_linear_fwd_bm with a row limit of its own: the same kernel, chain, carry tiles and epilogue; its
// expansion policy ExpandBM brings its own loads (a chunk is 0 to 8 halfwords at an arbitrary 2-byte offset whose address comes from
// the metadata, which is therefore fetched one batch further ahead than the values) and its own batch registers.
#include "common.hpp"
#include "expand_bm.hpp"
#include "expand_nm.hpp"
#include "mfma.hpp"

// rows of X the packed kernel takes: chosen from tools/bench_linear24.py (profiles/linear24.md); a multiple of 16 in 16..64
#ifndef VLMC_LINEAR24_MAX_ROWS
#define VLMC_LINEAR24_MAX_ROWS 64
#endif
static_assert(VLMC_LINEAR24_MAX_ROWS % 16 == 0 && VLMC_LINEAR24_MAX_ROWS >= 16 && VLMC_LINEAR24_MAX_ROWS <= 64, "16, 32, 48 or 64");

// the bitmap format's own limit, chosen from tools/bench_linear24.py --format bm (profiles/linearbm.md); a multiple of 16 in 16..64
#ifndef VLMC_LINEARBM_MAX_ROWS
#define VLMC_LINEARBM_MAX_ROWS 16
#endif
static_assert(VLMC_LINEARBM_MAX_ROWS % 16 == 0 && VLMC_LINEARBM_MAX_ROWS >= 16 && VLMC_LINEARBM_MAX_ROWS <= 64, "16, 32, 48 or 64");

// most rows of X the Python wrappers give to the TILED packed kernel (gemm_nt.hip: gemm_nt_kernel<.., PackedNM<..>>, both n:m formats) above
// VLMC_LINEAR24_MAX_ROWS: chosen from tools/bench_linear24.py --tiled (profiles/linear_nm_tiled.md); 0 = never, else >= that limit
#ifndef VLMC_LINEAR_NM_TILED_MAX_ROWS
#define VLMC_LINEAR_NM_TILED_MAX_ROWS 0
#endif
static_assert(VLMC_LINEAR_NM_TILED_MAX_ROWS == 0 || VLMC_LINEAR_NM_TILED_MAX_ROWS >= VLMC_LINEAR24_MAX_ROWS, "0 (never) or at least the packed kernel's own limit");

// the same for the bitmap format (gemm_nt_kernel<.., PackedBM>) above VLMC_LINEARBM_MAX_ROWS: chosen from tools/bench_linear24.py --tiled
// --format bm (profiles/linearbm_tiled.md); 0 = never, else >= that limit
#ifndef VLMC_LINEARBM_TILED_MAX_ROWS
#define VLMC_LINEARBM_TILED_MAX_ROWS 0
#endif
static_assert(VLMC_LINEARBM_TILED_MAX_ROWS == 0 || VLMC_LINEARBM_TILED_MAX_ROWS >= VLMC_LINEARBM_MAX_ROWS, "0 (never) or at least the packed kernel's own limit");

namespace vlmc {

constexpr int L24_WAVES = 16;

// gemm_nt.hip: the register-staged tiled GEMM with the weight operand packed n:m (fmt 24 or 48), arguments checked here
int linear_nm_tiled_launch(const char *fn, int fmt, const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype,
                           int64_t M, int64_t N, int64_t K, int64_t ldx, void *Y, int64_t ldy, void *stream);

// gemm_nt.hip: the same kernel with the weight operand bitmap-packed, arguments checked here
int linear_bm_tiled_launch(const char *fn, const void *X, const void *values, const uint8_t *meta, const uint16_t *offs, const int64_t *rowptr,
                           int64_t nnz, const void *bias, int dtype, int64_t M, int64_t N, int64_t K, int64_t ldx, void *Y, int64_t ldy,
                           void *stream);

struct Linear24Args {
    const uint16_t *X;            // [M, K], row stride ldx
    const uint16_t *values;       // [N, K / 2]
    const uint8_t *meta;          // [N, K / 8]
    const uint16_t *bias;         // [N] or NULL
    uint16_t *Y;                  // [M, N], row stride ldy
    int64_t ldx, ldy;
    int M, N, K;
};
struct LinearBMArgs : Linear24Args {                                 // values: [nnz + 16]
    const uint16_t *offs;         // [N, ceil(K / 32)]
    const int64_t *rowptr;        // [N + 1]
    int64_t nnz;
};

// The expansion policies: how the packed bytes of one chunk become the 8 weights of the A fragment (expand_nm.hpp: expand24,
// perm_selector and the selector table).  A policy owns its loads and
// its batch registers:
//   Args         the kernel's arguments (Linear24Args, or more)
//   steps<MT>()  the K-steps of a batch -- what a wave holds in registers at MT tiles of X
//   Regs<D>      the weight side of a batch
//   init         once per workgroup, before the kernel's first barrier;   row: this lane's row of W
//   load         issue the loads of chunk cc into step d and `prime` chunk `ahead`: what must be in flight one batch earlier (the
//                kernel hands both over clamped: a chunk past K is chunk 0, loaded whatever happens and zeroed when used)
//   expand       step d -> the fragment;   spare: >= N readable halfwords, loaded in the place of a missing bias
// The two n:m formats share everything but `expand`: a chunk is 8 bytes of values and 1 byte of meta at an address K alone fixes.
struct ExpandNM {
    using Args = Linear24Args;
    template <int MT> static constexpr int steps() { return MT == 1 ? 8 : (MT == 2 ? 4 : 2); }
    template <int D> struct Regs {
        u32x2_t v[D];
        uint32_t code[D];
    };
    const uint16_t *vrow;
    const uint8_t *mrow;
    int chunks;
    static __device__ __forceinline__ const uint16_t *spare(const Args &a) { return a.values; }
    __device__ __forceinline__ void row(const Args &a, int wrow, int) {
        chunks = a.K >> 3;
        vrow = a.values + int64_t(wrow) * (a.K >> 1);
        mrow = a.meta + int64_t(wrow) * chunks;
    }
    template <int D> __device__ __forceinline__ void prime(Regs<D> &, int, int) const {}
    template <int D> __device__ __forceinline__ void load(Regs<D> &R, int d, int cc, int) const {
        R.v[d] = *reinterpret_cast<const u32x2_t *>(vrow + cc * 4);
        R.code[d] = mrow[cc];
    }
};

struct Expand24 : ExpandNM {
    __device__ __forceinline__ void init(int) {}
    template <int D> __device__ __forceinline__ u32x4_t expand(const Regs<D> &R, int d) const { return expand24(R.v[d], R.code[d]); }
};

// 4:8: bit j of the byte says that position j holds the next value.  The chunk's 8 bytes are exactly the sources of v_perm_b32
// ({v[1], v[0]}: selector s picks byte s of the chunk, 0x0c gives 0x00), so each output dword is one perm whose selector comes
// from a table byte -> four selector dwords (4 KiB of LDS, filled here).  A selector never names anything but a byte of the
// chunk or zero, and the table is indexed by a byte: whatever the metadata holds, nothing outside the chunk is read.  A byte
// with more than four bits set places the chunk's four values at its lowest four set bits and zeros at the others.
struct Expand48 : ExpandNM {
    const u32x4_t *sel;
    __device__ __forceinline__ void init(int tid) {
        __shared__ u32x4_t table[256];
        fill_perm_table<64 * L24_WAVES, 0>(reinterpret_cast<uint32_t *>(table), tid);   // 256 entries x 4 dwords
        sel = table;
    }
    template <int D> __device__ __forceinline__ u32x4_t expand(const Regs<D> &R, int d) const {
        return expand48(R.v[d], sel[R.code[d] & 0xffu]);
    }
};
static_assert(64 * L24_WAVES == 256 * 4, "Expand48 / ExpandBM::init: one thread per selector dword (fill_perm_table<1024>)");

// bm (expand_bm.hpp: the index lookup, the five-dword load, the shift and the two selector tables): a chunk is 0 to 8 halfwords at an
// arbitrary 2-byte offset whose address depends on meta and offs, so those are fetched ONE BATCH FURTHER AHEAD (`prime`): when a wave
// hands on and issues its next batch's value loads, that batch's metadata arrived a whole round ago, and the metadata of the batch
// after goes out with them.
struct ExpandBM : BMRow {
    using Args = LinearBMArgs;
    template <int MT> static constexpr int steps() { return MT <= 2 ? 4 : 2; }
    template <int D> using Regs = BMRegs<D>;
    static __device__ __forceinline__ const uint16_t *spare(const Args &a) { return a.offs; }
    __device__ __forceinline__ void init(int tid) {
        __shared__ u32x4_t table[512];
        fill_bm_tables<64 * L24_WAVES>(table, tid);
        sel = table;
    }
    __device__ __forceinline__ void row(const Args &a, int wrow, int fq) { BMRow::row(a.values, a.meta, a.offs, a.rowptr, a.nnz, a.N, a.K, wrow, fq); }
};

// MT tiles of 16 rows of X; D K-steps per batch (what a wave holds in registers); E the format's expansion policy
template <typename T, int MT, typename E>
__global__ __launch_bounds__(64 * L24_WAVES) void linear24_kernel(const typename E::Args a) {
    constexpr int D = E::template steps<MT>();
    __shared__ f32x4_t carry[MT][64];
    __shared__ int turn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;             // fragment: row (lane & 15), k = 8 * (lane >> 4) + j
    const int n0 = blockIdx.x * 16;
    const int chunks = a.K >> 3, nb = (chunks + 4 * D - 1) / (4 * D);
    E expand;
    expand.init(tid);
    if (tid == 0) turn = 0;
    __syncthreads();

    // rows past the end are clamped to the last one: their products are never stored
    expand.row(a, min(n0 + fr, a.N - 1), fq);
    const uint16_t *xrow[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) xrow[t] = a.X + int64_t(min(t * 16 + fr, a.M - 1)) * a.ldx;
    const int nl = n0 + fq * 4;                            // this lane's four output features
    // (clamped and never branched round, so that nothing waits for them before the epilogue: without a bias four halfwords of
    // the packed weight are loaded in its place and ignored)
    const uint16_t *bsrc = a.bias != nullptr ? a.bias : E::spare(a);
    uint16_t braw[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) braw[r] = bsrc[min(nl + r, a.N - 1)];

    struct Batch {
        typename E::template Regs<D> w;
        u32x4_t x[MT][D];
    };
    // every load is issued whatever the chunk: one past K reads chunk 0 and is zeroed when used (no branch round a load)
    auto load = [&](int b, Batch &B) {
        const int ahead = min(b + L24_WAVES, nb - 1);     // this wave's batch after b: what the policy may have to prime
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int c = (b * D + d) * 4 + fq, cc = c < chunks ? c : 0, ca = (ahead * D + d) * 4 + fq;
            expand.load(B.w, d, cc, ca < chunks ? ca : 0);
#pragma unroll
            for (int t = 0; t < MT; ++t) B.x[t][d] = *reinterpret_cast<const u32x4_t *>(xrow[t] + cc * 8);
        }
    };

    Batch cur;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const int c = (min(wave, nb - 1) * D + d) * 4 + fq;
        expand.prime(cur.w, d, c < chunks ? c : 0);
    }
    load(min(wave, nb - 1), cur);
    for (int b = wave; b < nb; b += L24_WAVES) {
        const u32x4_t zero = {0u, 0u, 0u, 0u};
        u32x4_t wf[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const bool ok = (b * D + d) * 4 + fq < chunks;
            wf[d] = ok ? expand.expand(cur.w, d) : zero;
#pragma unroll
            for (int t = 0; t < MT; ++t) cur.x[t][d] = ok ? cur.x[t][d] : zero;
        }
        // ---- this wave's turn: the chain so far, D more steps, hand on ------------------------------------------------
        while (__hip_atomic_load(&turn, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != b) __builtin_amdgcn_s_sleep(1);
        f32x4_t acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = b == 0 ? f32x4_t{0.f, 0.f, 0.f, 0.f} : carry[t][lane];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[t] = mfma16<T>(wf[d], cur.x[t][d], acc[t]);
        if (b + 1 < nb) {
#pragma unroll
            for (int t = 0; t < MT; ++t) carry[t][lane] = acc[t];
            __hip_atomic_store(&turn, b + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            load(min(b + L24_WAVES, nb - 1), cur);        // in flight while the other fifteen waves take their turns
            continue;
        }
        // accumulator register r of a lane: feature nl + r (the A row), row t * 16 + fr of X (the B column)
        const bool vec_ok = (a.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Y) & 7u) == 0;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = t * 16 + fr;
            if (m >= a.M || nl >= a.N) continue;
            uint16_t o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = from_f32<T>(a.bias != nullptr ? acc[t][r] + to_f32<T>(braw[r]) : acc[t][r]);
            uint16_t *dst = a.Y + int64_t(m) * a.ldy + nl;
            if (vec_ok && nl + 3 < a.N) {
                const u32x2_t v = {uint32_t(o[0]) | uint32_t(o[1]) << 16, uint32_t(o[2]) | uint32_t(o[3]) << 16};
                *reinterpret_cast<u32x2_t *>(dst) = v;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (nl + r < a.N) dst[r] = o[r];
            }
        }
    }
}

template <typename T, typename E> static void launch_linear24(const typename E::Args &a, hipStream_t s) {
    const dim3 grid(unsigned((a.N + 15) / 16)), block(64 * L24_WAVES);
    switch ((a.M + 15) / 16) {
        case 1: VLMC_LAUNCH_TIMED((linear24_kernel<T, 1, E>), grid, block, s, a); break;
        case 2: VLMC_LAUNCH_TIMED((linear24_kernel<T, 2, E>), grid, block, s, a); break;
        case 3: VLMC_LAUNCH_TIMED((linear24_kernel<T, 3, E>), grid, block, s, a); break;
        default: VLMC_LAUNCH_TIMED((linear24_kernel<T, 4, E>), grid, block, s, a); break;
    }
}

// the dense weight, then 16 bytes for the unpack kernel's bad-group counter (never read: meta is trusted here)
static size_t linear24_dense_bytes(int64_t N, int64_t K) { return round_up(size_t(N) * size_t(K) * 2, 16); }

}  // namespace vlmc

using namespace vlmc;

extern "C" int vlmc_linear_fwd_24_max_rows(void) { return VLMC_LINEAR24_MAX_ROWS; }

extern "C" size_t vlmc_linear_fwd_24_workspace(int64_t M, int64_t N, int64_t K) {
    if (M <= VLMC_LINEAR24_MAX_ROWS || N <= 0 || K <= 0) return 0;
    return linear24_dense_bytes(N, K) + 16;
}

extern "C" int vlmc_linear_fwd_bm_max_rows(void) { return VLMC_LINEARBM_MAX_ROWS; }

// the same quantity above the bitmap format's own limit
extern "C" size_t vlmc_linear_fwd_bm_workspace(int64_t M, int64_t N, int64_t K) {
    if (M <= VLMC_LINEARBM_MAX_ROWS || N <= 0 || K <= 0) return 0;
    return linear24_dense_bytes(N, K) + 16;
}

// what every packed entry point asks of the arguments they share; `fn` names the export in every error
static int linear_packed_check(const char *fn, const void *X, const void *values, const uint8_t *meta, int dtype, int64_t M, int64_t N, int64_t K,
                               int64_t ldx, const void *Y, int64_t ldy) {
    VLMC_REQUIRE(dtype == VLMC_F16 || dtype == VLMC_BF16, "%s: dtype must be VLMC_F16 or VLMC_BF16", fn);
    VLMC_REQUIRE(X && values && meta && Y, "%s: null pointer", fn);
    VLMC_REQUIRE(M > 0 && N > 0 && K > 0 && M < (int64_t(1) << 31) && N < (int64_t(1) << 31) && K < (int64_t(1) << 31), "%s: bad shape", fn);
    VLMC_REQUIRE(K % 8 == 0 && ldx % 8 == 0 && ldx >= K && ldy >= N,
                 "%s: K and the row stride of X must be multiples of 8 elements, ldx >= K, ldy >= N", fn);
    return VLMC_OK;
}

template <typename E> static int linear_packed_launch(const char *fn, const typename E::Args &a, int dtype, void *stream) {
    if (dtype == VLMC_BF16) launch_linear24<bf16_t, E>(a, as_stream(stream));
    else launch_linear24<f16_t, E>(a, as_stream(stream));
    VLMC_HIP_CHECK_LAUNCH(fn);
    return VLMC_OK;
}

// the one entry point behind both formats: `fn` names the export in every error, `unpack` is the format's unpack export
template <typename E>
static int linear_packed_fwd(const char *fn, int (*unpack)(const void *, const uint8_t *, int, int64_t, int64_t, void *, int64_t, uint8_t *, int64_t,
                                                           unsigned int *, void *),
                             const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype, int64_t M, int64_t N, int64_t K,
                             int64_t ldx, void *Y, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream) {
    const int ok = linear_packed_check(fn, X, values, meta, dtype, M, N, K, ldx, Y, ldy);
    if (ok != VLMC_OK) return ok;
    VLMC_REQUIRE(aligned16(X) && (reinterpret_cast<uintptr_t>(values) & 7u) == 0, "%s: X must be 16-byte, values 8-byte aligned", fn);
    if (M > VLMC_LINEAR24_MAX_ROWS) {
        const size_t dense = linear24_dense_bytes(N, K);
        VLMC_REQUIRE(workspace != nullptr && workspace_bytes >= dense + 16 && aligned16(workspace),
                     "%s: M > %d needs a 16-byte aligned workspace of vlmc_linear_fwd_24_workspace() bytes", fn, VLMC_LINEAR24_MAX_ROWS);
        unsigned int *bad = reinterpret_cast<unsigned int *>(static_cast<unsigned char *>(workspace) + dense);
        const int rc = unpack(values, meta, dtype, N, K, workspace, K, nullptr, 0, bad, stream);
        if (rc != VLMC_OK) return rc;
        return vlmc_linear_fwd(X, workspace, bias, dtype, M, N, K, ldx, K, Y, ldy, stream);
    }
    const Linear24Args a{static_cast<const uint16_t *>(X), static_cast<const uint16_t *>(values), meta, static_cast<const uint16_t *>(bias),
                         static_cast<uint16_t *>(Y), ldx, ldy, int(M), int(N), int(K)};
    return linear_packed_launch<E>(fn, a, dtype, stream);
}

extern "C" int vlmc_linear_fwd_24(const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype, int64_t M, int64_t N,
                                  int64_t K, int64_t ldx, void *Y, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream) {
    return linear_packed_fwd<Expand24>("vlmc_linear_fwd_24", vlmc_unpack_24, X, values, meta, bias, dtype, M, N, K, ldx, Y, ldy, workspace,
                                       workspace_bytes, stream);
}

extern "C" int vlmc_linear_fwd_48(const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype, int64_t M, int64_t N,
                                  int64_t K, int64_t ldx, void *Y, int64_t ldy, void *workspace, size_t workspace_bytes, void *stream) {
    return linear_packed_fwd<Expand48>("vlmc_linear_fwd_48", vlmc_unpack_48, X, values, meta, bias, dtype, M, N, K, ldx, Y, ldy, workspace,
                                       workspace_bytes, stream);
}

// the tiled kernel at any M: no workspace, no row limit of its own
static int linear_nm_tiled(const char *fn, int fmt, const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype, int64_t M,
                           int64_t N, int64_t K, int64_t ldx, void *Y, int64_t ldy, void *stream) {
    const int ok = linear_packed_check(fn, X, values, meta, dtype, M, N, K, ldx, Y, ldy);
    if (ok != VLMC_OK) return ok;
    VLMC_REQUIRE(aligned16(X) && (reinterpret_cast<uintptr_t>(values) & 7u) == 0, "%s: X must be 16-byte, values 8-byte aligned", fn);
    return linear_nm_tiled_launch(fn, fmt, X, values, meta, bias, dtype, M, N, K, ldx, Y, ldy, stream);
}

extern "C" int vlmc_linear_fwd_24_tiled_max_rows(void) { return VLMC_LINEAR_NM_TILED_MAX_ROWS; }

extern "C" int vlmc_linear_fwd_24_tiled(const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype, int64_t M, int64_t N,
                                        int64_t K, int64_t ldx, void *Y, int64_t ldy, void *stream) {
    return linear_nm_tiled("vlmc_linear_fwd_24_tiled", 24, X, values, meta, bias, dtype, M, N, K, ldx, Y, ldy, stream);
}

extern "C" int vlmc_linear_fwd_48_tiled(const void *X, const void *values, const uint8_t *meta, const void *bias, int dtype, int64_t M, int64_t N,
                                        int64_t K, int64_t ldx, void *Y, int64_t ldy, void *stream) {
    return linear_nm_tiled("vlmc_linear_fwd_48_tiled", 48, X, values, meta, bias, dtype, M, N, K, ldx, Y, ldy, stream);
}

// what both bitmap entry points ask of their arguments beyond linear_packed_check
static int linear_bm_check(const char *fn, const void *X, const void *values, const uint8_t *meta, const uint16_t *offs, const int64_t *rowptr,
                           int64_t nnz, int dtype, int64_t M, int64_t N, int64_t K, int64_t ldx, const void *Y, int64_t ldy) {
    const int ok = linear_packed_check(fn, X, values, meta, dtype, M, N, K, ldx, Y, ldy);
    if (ok != VLMC_OK) return ok;
    VLMC_REQUIRE(offs && rowptr, "%s: null pointer", fn);
    VLMC_REQUIRE(K <= 65536 && nnz >= 0 && nnz <= N * K, "%s: K must be at most 65536 and 0 <= nnz <= N * K", fn);
    VLMC_REQUIRE(aligned16(X) && (reinterpret_cast<uintptr_t>(values) & 3u) == 0 && (reinterpret_cast<uintptr_t>(meta) & 3u) == 0,
                 "%s: X must be 16-byte, values and meta 4-byte aligned", fn);
    return VLMC_OK;
}

extern "C" int vlmc_linear_fwd_bm(const void *X, const void *values, const uint8_t *meta, const uint16_t *offs, const int64_t *rowptr, int64_t nnz,
                                  const void *bias, int dtype, int64_t M, int64_t N, int64_t K, int64_t ldx, void *Y, int64_t ldy, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    const char *fn = "vlmc_linear_fwd_bm";
    const int ok = linear_bm_check(fn, X, values, meta, offs, rowptr, nnz, dtype, M, N, K, ldx, Y, ldy);
    if (ok != VLMC_OK) return ok;
    if (M > VLMC_LINEARBM_MAX_ROWS) {
        const size_t dense = linear24_dense_bytes(N, K);
        VLMC_REQUIRE(workspace != nullptr && workspace_bytes >= dense + 16 && aligned16(workspace),
                     "%s: M > %d needs a 16-byte aligned workspace of vlmc_linear_fwd_bm_workspace() bytes", fn, VLMC_LINEARBM_MAX_ROWS);
        unsigned int *bad = reinterpret_cast<unsigned int *>(static_cast<unsigned char *>(workspace) + dense);
        const int rc = vlmc_unpack_bm(values, meta, offs, rowptr, nnz, dtype, N, K, workspace, K, nullptr, 0, bad, stream);
        if (rc != VLMC_OK) return rc;
        return vlmc_linear_fwd(X, workspace, bias, dtype, M, N, K, ldx, K, Y, ldy, stream);
    }
    const LinearBMArgs a{{static_cast<const uint16_t *>(X), static_cast<const uint16_t *>(values), meta, static_cast<const uint16_t *>(bias),
                          static_cast<uint16_t *>(Y), ldx, ldy, int(M), int(N), int(K)}, offs, rowptr, nnz};
    return linear_packed_launch<ExpandBM>(fn, a, dtype, stream);
}

extern "C" int vlmc_linear_fwd_bm_tiled_max_rows(void) { return VLMC_LINEARBM_TILED_MAX_ROWS; }

// the tiled kernel at any M: no workspace, no row limit of its own
extern "C" int vlmc_linear_fwd_bm_tiled(const void *X, const void *values, const uint8_t *meta, const uint16_t *offs, const int64_t *rowptr,
                                        int64_t nnz, const void *bias, int dtype, int64_t M, int64_t N, int64_t K, int64_t ldx, void *Y, int64_t ldy,
                                        void *stream) {
    const char *fn = "vlmc_linear_fwd_bm_tiled";
    const int ok = linear_bm_check(fn, X, values, meta, offs, rowptr, nnz, dtype, M, N, K, ldx, Y, ldy);
    if (ok != VLMC_OK) return ok;
    return linear_bm_tiled_launch(fn, X, values, meta, offs, rowptr, nnz, bias, dtype, M, N, K, ldx, Y, ldy, stream);
}
