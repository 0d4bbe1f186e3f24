// Per-bin statistics of the subband stream over a window of the last T hops (apv_stream_set_stat_hops):
//   R_B[k] = sum_t X_B^(h-t)[k]^H X_B^(h-t)[k],  R_D likewise,  r[k] = sum_t X_B^(h-t)[k]^H d^(h-t)[k],  t = 0 .. T-1
// (the per-bin form of the reference's statistics buffer, Python/apvast.py:329-364, which spans several blocks).
//
//   statwin_kernel   per (bin, matrix, zone program): the hop's own Gram matrix G = X^H X (and g = X_B^H d) on the matrix cores,
//                    written to slot `head` of a ring of T slots, then the window sum of the slots IN THE ORDER OF AGE (oldest
//                    first, the new hop last) into the explicit-statistics arrays the joint diagonalisation reads.  The order
//                    does not depend on where the ring stands, so a resumed stream and the whole-signal call sum the same bits.
//   statwin_advance  one thread: head <- (head + 1) mod T, fill <- min(fill + 1, T).  The two words live in device memory, so a
//                    captured hop graph replays unchanged whatever the ring's phase is.
//
//   statforget_kernel  the same Gram matrices, added to ONE slot that forgets exponentially (apv_stream_set_stat_forgetting):
//                    R <- beta R + G, r <- beta r + g, one fma per real and per imaginary part by the lane that owns the
//                    element; the new sums go back to the slot and, full, to the explicit-statistics arrays.  No counters.
//
// Ring slot of one bin: [R_B: L x L][R_D: L x L][r: L] complex of the compute precision; a zone program's ring is [T][K][slot].
// Only the lower triangle of a matrix is kept in the ring (tiles on and below the diagonal; inside a diagonal tile the elements
// with j <= i); the sums are written out full, the upper triangle as the conjugate of the lower, the diagonal real.
#include "apv_internal.h"

namespace {

using d4w = __attribute__((ext_vector_type(4))) double;
using f4w = __attribute__((ext_vector_type(4))) float;

// 16 x 16 x 4 MFMA of either precision.  Operands of both: lane (c = lane & 15, h = lane >> 4) supplies A[i = c][k = h] and
// B[k = h][j = c].  Accumulator element t of that lane is column c of row  h + 4 t (f64)  |  4 h + t (f32).
template <typename T> struct Mma;
template <> struct Mma<double> {
    using v4 = d4w;
    using cplx = double2;
    static __device__ __forceinline__ v4 mfma(double a, double b, v4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int h, int t) { return h + 4 * t; }
    static __device__ __forceinline__ cplx make(double x, double y) { return make_double2(x, y); }
};
template <> struct Mma<float> {
    using v4 = f4w;
    using cplx = float2;
    static __device__ __forceinline__ v4 mfma(float a, float b, v4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int h, int t) { return 4 * h + t; }
    static __device__ __forceinline__ cplx make(float x, float y) { return make_float2(x, y); }
};

struct StatWinArgs {
    int K, M, L, T, NT;          // NT = ceil(L / 16) tiles per side
    const void* XB[2];           // per zone program of the launch: bin-major slabs [K][M][L], target [K][M]
    const void* XD[2];
    const void* d[2];
    void* ring[2];               // [T][K][2 L L + L]
    void* RB[2];                 // window sums: [K][L][L], [K][L][L], [K][L]
    void* RD[2];
    void* r[2];
    const int32_t* ctr;          // {head: slot the new hop goes to, fill: slots that hold a hop, <= T}
};

// the window sum of one element: the `nold` older slots oldest first, then the hop's own value, which also goes to slot `head`
template <typename C, typename T>
__device__ __forceinline__ C window_sum(C* __restrict__ ring, size_t slot_stride, size_t idx, int head, int nold, int Tn, T gx, T gy) {
    T sx = 0, sy = 0;
    int slot = head - nold;
    if (slot < 0) slot += Tn;
    for (int a = 0; a < nold; ++a) {
        const C v = ring[(size_t)slot * slot_stride + idx];
        sx += v.x;
        sy += v.y;
        if (++slot == Tn) slot = 0;
    }
    C g;
    g.x = gx; g.y = gy;
    ring[(size_t)head * slot_stride + idx] = g;
    C s;
    s.x = sx + gx; s.y = sy + gy;
    return s;
}

// what statwin_kernel does with an element of the hop's Gram matrices: the window sum over the ring, see window_sum
template <typename C, typename T>
struct WindowUpdate {
    C* __restrict__ ring;
    size_t slot_stride;
    int head, nold, Tn;
    __device__ __forceinline__ C operator()(size_t idx, T gx, T gy) const {
        return window_sum<C, T>(ring, slot_stride, idx, head, nold, Tn, gx, gy);
    }
};

// ... and what statforget_kernel does: acc <- beta acc + g, real and imaginary part each one fma
template <typename C, typename T>
struct ForgetUpdate {
    C* __restrict__ acc;
    T beta;
    __device__ __forceinline__ C operator()(size_t idx, T gx, T gy) const {
        const C old = acc[idx];
        C s;
        s.x = fma(beta, old.x, gx); s.y = fma(beta, old.y, gy);
        acc[idx] = s;
        return s;
    }
};

// The hop's Gram matrix of block (k = blockIdx.x, which = blockIdx.y, z = blockIdx.z) in 16 x 16 tiles on the matrix cores; every
// wave of the workgroup takes tiles wave, wave + n_waves, ... of the lower triangle.  Each element (and each entry of g = X_B^H d,
// from the tiles of column 0) goes through `upd` (index inside the zone program's slot, value) -> the statistic to write out.
template <typename XT, typename T, typename Upd>
__device__ __forceinline__ void gram_tiles(const StatWinArgs& a, const Upd& upd) {
    using MM = Mma<T>;
    using C = typename MM::cplx;
    const int k = blockIdx.x, which = blockIdx.y, z = blockIdx.z;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int L = a.L, M = a.M;
    const size_t E = 2 * (size_t)L * L + L;
    const XT* __restrict__ X = reinterpret_cast<const XT*>(which ? a.XD[z] : a.XB[z]) + (size_t)k * M * L;
    const XT* __restrict__ dv = reinterpret_cast<const XT*>(a.d[z]) + (size_t)k * M;
    C* __restrict__ R = reinterpret_cast<C*>(which ? a.RD[z] : a.RB[z]) + (size_t)k * L * L;
    C* __restrict__ rr = reinterpret_cast<C*>(a.r[z]) + (size_t)k * L;
    const size_t mat0 = (size_t)k * E + (which ? (size_t)L * L : 0), vec0 = (size_t)k * E + 2 * (size_t)L * L;
    const int n_tiles = a.NT * (a.NT + 1) / 2;
    for (int tile = wave; tile < n_tiles; tile += n_waves) {
        int ta = 0, tb = tile;
        while (tb > ta) { tb -= ta + 1; ++ta; }
        const int ia = 16 * ta + c, ib = 16 * tb + c;
        const bool oka = ia < L, okb = ib < L;
        const bool want_r = which == 0 && tb == 0;          // the tiles of column 0 cover every loudspeaker once
        typename MM::v4 re = {0, 0, 0, 0}, im = {0, 0, 0, 0};
        T rx = 0, ry = 0;
        // A[i = c][k = h] = conj(X[m0 + h][16 ta + c]), B[k = h][j = c] = X[m0 + h][16 tb + c]; rows and columns beyond M, L are zeros
        for (int m0 = 0; m0 < M; m0 += 4) {
            const int m = m0 + h;
            const bool okm = m < M;
            T ar = 0, ai = 0, br = 0, bi = 0, dx = 0, dy = 0;
            if (okm && oka) { const XT v = X[(size_t)m * L + ia]; ar = (T)v.x; ai = (T)v.y; }
            if (okm && okb) { const XT v = X[(size_t)m * L + ib]; br = (T)v.x; bi = (T)v.y; }
            if (okm && want_r) { const XT v = dv[m]; dx = (T)v.x; dy = (T)v.y; }
            re = MM::mfma(ar, br, re);
            re = MM::mfma(ai, bi, re);
            im = MM::mfma(ar, bi, im);
            im = MM::mfma(-ai, br, im);
            rx += ar * dx + ai * dy;
            ry += ar * dy - ai * dx;
        }
        auto emit = [&](int t, T gx, T gy) {
            const int i = 16 * ta + MM::row(h, t), j = ib;
            if (i >= L || j >= L || j > i) return;            // (j > i: upper part of a diagonal tile, mirrored from the lower)
            const C s = upd(mat0 + (size_t)i * L + j, gx, i == j ? (T)0 : gy);
            R[(size_t)i * L + j] = s;
            if (i != j) R[(size_t)j * L + i] = MM::make(s.x, -s.y);
        };
        emit(0, re[0], im[0]);
        emit(1, re[1], im[1]);
        emit(2, re[2], im[2]);
        emit(3, re[3], im[3]);
        if (want_r) {
            rx += __shfl_xor(rx, 16, 64); ry += __shfl_xor(ry, 16, 64);
            rx += __shfl_xor(rx, 32, 64); ry += __shfl_xor(ry, 32, 64);
            if (h == 0 && oka) rr[ia] = upd(vec0 + ia, rx, ry);
        }
    }
}

// grid (K, 2 matrices, zone programs)
template <typename XT, typename T>
__global__ void __launch_bounds__(256) statwin_kernel(const StatWinArgs a) {
    using C = typename Mma<T>::cplx;
    const int Tn = a.T, head = a.ctr[0], fill = a.ctr[1];
    const int nold = fill < Tn - 1 ? fill : Tn - 1;         // a full ring: the slot at `head` is the oldest and leaves the window
    const size_t slot_stride = (size_t)a.K * (2 * (size_t)a.L * a.L + a.L);
    gram_tiles<XT, T>(a, WindowUpdate<C, T>{reinterpret_cast<C*>(a.ring[blockIdx.z]), slot_stride, head, nold, Tn});
}

// the same grid; a.ring[z] is the one accumulator slot [K][2 L L + L], a.T and a.ctr are not read
template <typename XT, typename T>
__global__ void __launch_bounds__(256) statforget_kernel(const StatWinArgs a, const T beta) {
    using C = typename Mma<T>::cplx;
    gram_tiles<XT, T>(a, ForgetUpdate<C, T>{reinterpret_cast<C*>(a.ring[blockIdx.z]), beta});
}

__global__ void statwin_advance_kernel(int32_t* __restrict__ ctr, int Tn) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int head = ctr[0], fill = ctr[1];
        ctr[0] = head + 1 == Tn ? 0 : head + 1;
        ctr[1] = fill < Tn ? fill + 1 : Tn;
    }
}

__global__ void __launch_bounds__(256) widen_c64_kernel(size_t count, const float2* __restrict__ in, double2* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = make_double2((double)in[i].x, (double)in[i].y);
}

}  // namespace

size_t apv_statwin_slot_elems(int L) { return 2 * (size_t)L * L + L; }

// One hop of `zones` (1 | 2) zone programs: Gram matrices into the ring, window sums into RB / RD / r, counters advanced.
// x_c128: the slabs are c128 (else c64); acc_f64: ring and sums are c128, formed on the f64 MFMA (else c64 on the f32 MFMA).
hipError_t apv_launch_statwin(int x_c128, int acc_f64, int K, int M, int L, int T, int zones, const void* const* XB,
                              const void* const* XD, const void* const* d, void* const* ring, void* const* RB, void* const* RD,
                              void* const* r, int32_t* ctr, hipStream_t s) {
    if (K <= 0) return hipSuccess;
    if (L < 1 || L > APV_MAX_SRCS || M < 1 || T < 2 || T > APV_MAX_STAT_HOPS || zones < 1 || zones > 2 || !ctr) return hipErrorInvalidValue;
    StatWinArgs a{};
    a.K = K; a.M = M; a.L = L; a.T = T; a.NT = (L + 15) / 16;
    for (int z = 0; z < zones; ++z) {
        a.XB[z] = XB[z]; a.XD[z] = XD[z]; a.d[z] = d[z];
        a.ring[z] = ring[z]; a.RB[z] = RB[z]; a.RD[z] = RD[z]; a.r[z] = r[z];
    }
    a.ctr = ctr;
    const int n_tiles = a.NT * (a.NT + 1) / 2;
    const dim3 grid(K, 2, zones), block(64 * (n_tiles < 4 ? n_tiles : 4));
    if (acc_f64) {
        if (x_c128) hipLaunchKernelGGL((statwin_kernel<double2, double>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((statwin_kernel<float2, double>), grid, block, 0, s, a);
    } else {
        if (x_c128) hipLaunchKernelGGL((statwin_kernel<double2, float>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((statwin_kernel<float2, float>), grid, block, 0, s, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(statwin_advance_kernel, dim3(1), dim3(64), 0, s, ctr, T);
    return hipGetLastError();
}

// One hop of an exponentially forgetting stream: R <- beta R + G in the accumulators `acc` [K][2 L L + L], the new sums into
// RB / RD / r.  The arguments are apv_launch_statwin's, without a window length and without counters.
hipError_t apv_launch_statforget(int x_c128, int acc_f64, int K, int M, int L, double beta, int zones, const void* const* XB,
                                 const void* const* XD, const void* const* d, void* const* acc, void* const* RB, void* const* RD,
                                 void* const* r, hipStream_t s) {
    if (K <= 0) return hipSuccess;
    if (L < 1 || L > APV_MAX_SRCS || M < 1 || !(beta > 0.0 && beta <= 1.0) || zones < 1 || zones > 2) return hipErrorInvalidValue;
    StatWinArgs a{};
    a.K = K; a.M = M; a.L = L; a.T = 1; a.NT = (L + 15) / 16;
    for (int z = 0; z < zones; ++z) {
        a.XB[z] = XB[z]; a.XD[z] = XD[z]; a.d[z] = d[z];
        a.ring[z] = acc[z]; a.RB[z] = RB[z]; a.RD[z] = RD[z]; a.r[z] = r[z];
    }
    const int n_tiles = a.NT * (a.NT + 1) / 2;
    const dim3 grid(K, 2, zones), block(64 * (n_tiles < 4 ? n_tiles : 4));
    if (acc_f64) {
        if (x_c128) hipLaunchKernelGGL((statforget_kernel<double2, double>), grid, block, 0, s, a, beta);
        else hipLaunchKernelGGL((statforget_kernel<float2, double>), grid, block, 0, s, a, beta);
    } else {
        if (x_c128) hipLaunchKernelGGL((statforget_kernel<double2, float>), grid, block, 0, s, a, (float)beta);
        else hipLaunchKernelGGL((statforget_kernel<float2, float>), grid, block, 0, s, a, (float)beta);
    }
    return hipGetLastError();
}

hipError_t apv_launch_widen_c64(size_t count, const void* in, void* out, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(widen_c64_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, count, (const float2*)in, (double2*)out);
    return hipGetLastError();
}
