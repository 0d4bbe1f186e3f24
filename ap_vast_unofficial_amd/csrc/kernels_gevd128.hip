// Batched joint diagonalisation (GEVD) + variable-span filter at orders 65..128, float64 arithmetic.
//
// One workgroup (1024 threads) owns one bin.  A full c128 matrix of order 128 is 256 KB and LDS holds 160 KiB, so the kernel
// keeps ONE packed Hermitian lower triangle (n (n+1)/2 c128 = 132 KB at n = 128) on-chip and parks what it needs later in a
// per-(zone, bin) HBM slot of (2 n^2 + n) c128 (apv_gevd_spill_bytes):
//
//   slot [0, n^2)                 R_B in (fused path), then the Householder vectors (column-packed)
//   slot [n^2, 2 n^2)             R_D in, then the Cholesky factor L (column-packed, n (n+1)/2)
//   slot [2 n^2, 2 n^2 + n)       r in
//
// Stages (reference Python/apvast.py:20-36, 378-414; the generic kernel kernels_gevd.hip does the same job at n <= 64):
//   0  [fused]  R_B, R_D, r from the slabs by corr128_kernel (c64 or c128 spectra), written into the slot
//   1  R_D -> LDS, loading (REG_ABS, or REG_REL with the Lanczos spectral norm of the generic kernel), Cholesky in place;
//      L parked
//   2  R_B -> LDS (+ optional bright loading), C = L^-1 R_B L^-H in place (LAPACK zhegs2, lower; its per-column triangular
//      solves are deferred to one forward substitution over the rows, which is exact: column k is final once its solve has
//      run); r~ = L^-1 r rides along
//   3  C = Q T Q^H, T real tridiagonal (LAPACK zhetd2, lower); y = Q^H r~; the reflectors are parked
//   4  T = Z diag(lam) Z^T by implicit QL with shifts (EISPACK tql2), Z (real, n x 128 f64 = 128 KB) accumulated in LDS over the
//      space the packed matrix held.  QL meets exact clusters (an (L - M)-fold zero eigenvalue when M < L): its rotations are
//      orthogonal whatever the spectrum, and its deflation test is relative; 30 n QL iterations per bin are the cap (status 2)
//   5  lam descending; c = Z^T y; s_V = sum_{i<V} c_i / (lam_i + mu) z_i for every requested rank
//   6  w_V = L^-H Q s_V (the reflectors and L read back from the slot, L^-H by back substitution); with U requested the same
//      for every z_i
//
// Outputs follow the handle: w c64 / lam f32 when out_c128 = 0, c128 / f64 otherwise; U in the complex type of the compute
// dtype.  status 1 = loaded R_D (or R_B's bright loading) not positive definite: w, lam and U are zeros.  gfx950, wave 64.
#include "apv_internal.h"

#include <type_traits>

#include <cstdlib>

namespace {

constexpr int NM = 128;                  // largest order
constexpr int TPB = 1024;
constexpr int NPK = NM * (NM + 1) / 2;   // packed triangle, 8256 elements
constexpr int CT = 64;                   // correlation tile
constexpr int CMT = 16;                  // control-point rows staged per step of the correlation

struct Gevd128Args {
    int n, K, nV;
    int reg_mode;
    int out_c128;
    double reg_dark, reg_bright, mu;
    const void* RB[2];       // per zone program: explicit (compute dtype) or slot-resident (c128) inputs
    const void* RD[2];
    const void* r[2];
    size_t in_mat;           // elements from one bin's matrix to the next
    size_t in_vec;
    void* w[2];
    void* lam[2];
    int32_t* status[2];
    void* U;                 // zone 0 only (explicit path)
    double2* slot;           // [zones][K] slots of (2 n^2 + n) c128
    int ranks[NM];
    SpanParams span;         // GevdParams::span
};

struct Corr128Args {
    int K, M, n, n_tiles;
    const void* XB[2];
    const void* XD[2];
    const void* d[2];
    double2* out;            // slots: RB at 0, RD at n^2, r at 2 n^2
    size_t slot;             // elements per slot
    double2* RB;             // statistics path: separate outputs (out == nullptr)
    double2* RD;
    double2* rr;
};

__device__ __forceinline__ double2 c2(double x, double y) { return make_double2(x, y); }
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return c2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return c2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return c2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// a * conj(b)
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) { return c2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
// conj(a) * b
__device__ __forceinline__ double2 ccmul(double2 a, double2 b) { return c2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }
__device__ __forceinline__ double2 cscale(double2 a, double s) { return c2(a.x * s, a.y * s); }
__device__ __forceinline__ double2 cconj(double2 a) { return c2(a.x, -a.y); }
__device__ __forceinline__ double cabs2(double2 a) { return a.x * a.x + a.y * a.y; }

__device__ __forceinline__ double2 ld(const float2* p, size_t i) { const float2 v = p[i]; return c2(v.x, v.y); }
__device__ __forceinline__ double2 ld(const double2* p, size_t i) { return p[i]; }
__device__ __forceinline__ void st(float2* p, size_t i, double2 v) { p[i] = make_float2((float)v.x, (float)v.y); }
__device__ __forceinline__ void st(double2* p, size_t i, double2 v) { p[i] = v; }

__device__ __forceinline__ int pk(int i, int j) { return i * (i + 1) / 2 + j; }                 // row-packed lower, j <= i
__device__ __forceinline__ int colofs(int n, int j) { return j * n - j * (j - 1) / 2; }        // column-packed lower: column j

// ---------------- stage 0: R_B, R_D, r of the slabs, one 64 x 64 tile of one matrix per workgroup ----------------
// grid (lower tiles x 2 matrices, K, zones); thread (ty, tx) of 16 x 16 owns rows i0 + ty + 16 a, columns j0 + tx + 16 b.
// Off-diagonal tiles write their conjugate transpose too: R comes out full Hermitian.
template <typename XT>
__global__ void __launch_bounds__(256) corr128_kernel(const Corr128Args a) {
    __shared__ double2 sXi[CMT][CT];
    __shared__ double2 sXj[CMT][CT];
    __shared__ double2 sd[CMT];
    const int which = blockIdx.x & 1, tile = blockIdx.x >> 1;
    const int k = blockIdx.y, z = blockIdx.z;
    const int n = a.n, M = a.M;
    int ti = 0, tj = tile;
    while (tj > ti) { tj -= ti + 1; ++ti; }
    const int i0 = ti * CT, j0 = tj * CT;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const XT* X = reinterpret_cast<const XT*>(which ? a.XD[z] : a.XB[z]) + (size_t)k * M * n;
    const XT* dv = reinterpret_cast<const XT*>(a.d[z]) + (size_t)k * M;
    const bool do_r = which == 0 && tj == 0;
    double2 acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = c2(0, 0);
    double2 racc[4] = {c2(0, 0), c2(0, 0), c2(0, 0), c2(0, 0)};
    for (int m0 = 0; m0 < M; m0 += CMT) {
        for (int idx = tid; idx < CMT * CT; idx += 256) {
            const int mm = idx / CT, c = idx - mm * CT;
            const bool okm = m0 + mm < M;
            sXi[mm][c] = (okm && i0 + c < n) ? ld(X, (size_t)(m0 + mm) * n + i0 + c) : c2(0, 0);
            sXj[mm][c] = (okm && j0 + c < n) ? ld(X, (size_t)(m0 + mm) * n + j0 + c) : c2(0, 0);
        }
        if (do_r && tid < CMT) sd[tid] = (m0 + tid < M) ? ld(dv, (size_t)m0 + tid) : c2(0, 0);
        __syncthreads();
#pragma unroll 4
        for (int mm = 0; mm < CMT; ++mm) {
            double2 xi[4], xj[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                xi[p] = sXi[mm][ty + 16 * p];
                xj[p] = sXj[mm][tx + 16 * p];
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // conj(x_i) x_j
                    acc[p][q].x = fma(xi[p].x, xj[q].x, fma(xi[p].y, xj[q].y, acc[p][q].x));
                    acc[p][q].y = fma(xi[p].x, xj[q].y, fma(-xi[p].y, xj[q].x, acc[p][q].y));
                }
            if (do_r && tx == 0) {
                const double2 dm = sd[mm];
#pragma unroll
                for (int p = 0; p < 4; ++p) racc[p] = cadd(racc[p], ccmul(xi[p], dm));
            }
        }
        __syncthreads();
    }
    double2* R;
    double2* rr;
    if (a.out) {
        double2* sl = a.out + ((size_t)z * a.K + k) * a.slot;
        R = sl + (which ? (size_t)n * n : 0);
        rr = sl + 2 * (size_t)n * n;
    } else {
        R = (which ? a.RD : a.RB) + (size_t)k * n * n;
        rr = a.rr + (size_t)k * n;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = i0 + ty + 16 * p;
        if (i >= n) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + tx + 16 * q;
            if (j >= n) continue;
            R[(size_t)i * n + j] = acc[p][q];
            if (i0 != j0) R[(size_t)j * n + i] = cconj(acc[p][q]);
        }
        if (do_r && tx == 0) rr[i] = racc[p];
    }
}

// sum over the first 128 threads (waves 0 and 1) of v; every thread gets the total.  Two barriers.
__device__ __forceinline__ double sum128(double v, double* sScal, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (tid < 128 && (tid & 63) == 0) sScal[tid >> 6] = v;
    __syncthreads();
    const double t = sScal[0] + sScal[1];
    __syncthreads();
    return t;
}

// spectral norm of the Hermitian PSD matrix held packed in sP: the largest Ritz value of up to n Lanczos steps from a start
// vector with no symmetry, then the top eigenvalue of the tridiagonal matrix by nine passes of 64-way multisection on Sturm
// counts (the definition of kernels_gevd.hip, so that oracle/subband.py matches)
__device__ double norm2_packed(const double2* sP, int n, double* sAl, double* sBe, double* sRow, double2* sVec, int* sMs, int tid) {
    double2 vcur = c2(0, 0), vprev = c2(0, 0);
    {
        const double f = (double)tid * 0.6180339887498949;
        if (tid < n) vcur = c2(1.0 + (f - floor(f)), 0.0);
        if (tid < n) sRow[tid] = cabs2(vcur);
        __syncthreads();
        double s2 = 0;
        for (int j = 0; j < n; ++j) s2 += sRow[j];
        vcur = cscale(vcur, 1.0 / sqrt(s2));
        __syncthreads();
    }
    double beta_prev = 0;
    int m = 0;
    for (int it = 0; it < n; ++it) {
        if (tid < n) sVec[tid] = vcur;
        __syncthreads();
        double2 y = c2(0, 0);
        if (tid < n) {
            for (int j = 0; j <= tid; ++j) y = cadd(y, cmul(sP[pk(tid, j)], sVec[j]));
            for (int j = tid + 1; j < n; ++j) y = cadd(y, ccmul(sP[pk(j, tid)], sVec[j]));
            sRow[tid] = vcur.x * y.x + vcur.y * y.y;
        }
        __syncthreads();
        double alpha = 0;
        for (int j = 0; j < n; ++j) alpha += sRow[j];
        __syncthreads();
        const double2 w = csub(csub(y, cscale(vcur, alpha)), cscale(vprev, beta_prev));
        if (tid < n) sRow[tid] = cabs2(w);
        if (tid == 0) sAl[it] = alpha;
        __syncthreads();
        double b2 = 0;
        for (int j = 0; j < n; ++j) b2 += sRow[j];
        const double beta = sqrt(b2);
        if (tid == 0) sBe[it] = beta;
        m = it + 1;
        __syncthreads();
        if (!(beta > 1e-14 * fabs(alpha)) || it + 1 == n) break;
        vprev = vcur;
        vcur = cscale(w, 1.0 / beta);
        beta_prev = beta;
    }
    double lo = 0, hi = 0;
    for (int i = 0; i < m; ++i) {
        const double r = (i > 0 ? sBe[i - 1] : 0.0) + (i + 1 < m ? sBe[i] : 0.0);
        hi = fmax(hi, sAl[i] + r);
    }
    for (int pass = 0; pass < 9 && hi > lo; ++pass) {
        const int t = tid & 63;
        const double x = lo + (hi - lo) * (double)(t + 1) / 65.0;
        int below = 0;
        constexpr double kTiny = 2.2250738585072014e-308;
        double dq = sAl[0] - x;
        below += !(dq >= 0.0);
        for (int i = 1; i < m; ++i) {
            if (fabs(dq) < kTiny) dq = dq < 0.0 ? -kTiny : kTiny;
            dq = sAl[i] - x - sBe[i - 1] * sBe[i - 1] / dq;
            below += !(dq >= 0.0);
        }
        __syncthreads();
        if (tid < 64) sMs[t] = (below < m) ? 1 : 0;
        __syncthreads();
        int q = 0;
        for (int j = 0; j < 64; ++j) q += sMs[j];
        const double step = (hi - lo) / 65.0;
        const double nlo = lo + step * (double)q, nhi = lo + step * (double)(q + 1);
        lo = nlo;
        hi = q < 64 ? nhi : hi;
        __syncthreads();
    }
    return 0.5 * (lo + hi);
}

// LDS plan (bytes): packed matrix / Z 132096, reduction rows 16384, four c128 vectors 8192, five f64 vectors 5120, ints 768,
// scalars 128 = 162688 of the CU's 163840
constexpr int LDS_BYTES = NPK * 16 + 8 * NM * 16 + 4 * NM * 16 + 5 * NM * 8 + (NM + 64) * 4 + 16 * 8;

// SPAN: the instantiation of launches with a span (gevd_span.h); the other one holds none of its code
template <typename RT, bool SPAN>
__global__ void __launch_bounds__(TPB) gevd128_kernel(const Gevd128Args a) {
    extern __shared__ __align__(16) unsigned char lds[];
    double2* const sP = reinterpret_cast<double2*>(lds);
    double* const sZ = reinterpret_cast<double*>(lds);          // stage 4 on: Z[i][q] at i * NM + q
    double2* const sRed = sP + NPK;                               // [8][NM]
    double2* const sR = sRed + 8 * NM;                            // r~, then y = Q^H r~
    double2* const sU = sR + NM;
    double2* const sLc = sU + NM;
    double2* const sTau = sLc + NM;
    double* const sD = reinterpret_cast<double*>(sTau + NM);
    double* const sE = sD + NM;
    double* const sLam = sE + NM;
    double* const sCs = sLam + NM;                                // L's diagonal (stages 1-2), then the QL rotations' c
    double* const sSn = sCs + NM;
    int* const sOrd = reinterpret_cast<int*>(sSn + NM);
    int* const sMisc = sOrd + NM;                                 // [64]
    double* const sScal = reinterpret_cast<double*>(sMisc + 64);  // [16]

    const int n = a.n, tid = threadIdx.x, k = blockIdx.x, z = blockIdx.y;
    const int rg = tid >> 7, cl = tid & 127;                      // row group (8) and column lane (128)
    const RT* RB = reinterpret_cast<const RT*>(a.RB[z]) + (size_t)k * a.in_mat;
    const RT* RD = reinterpret_cast<const RT*>(a.RD[z]) + (size_t)k * a.in_mat;
    const RT* rin = a.r[z] ? reinterpret_cast<const RT*>(a.r[z]) + (size_t)k * a.in_vec : nullptr;
    double2* const slot = a.slot + ((size_t)z * a.K + k) * (2 * (size_t)n * n + n);
    double2* const gV = slot;                                     // reflectors, column-packed
    double2* const gL = slot + (size_t)n * n;                     // L, column-packed
    int status = 0;

    // ---------------- stage 1: R_D, loading, Cholesky ----------------
    if (tid < n) sR[tid] = rin ? ld(rin, tid) : c2(0, 0);
    for (int i = rg; i < n; i += 8)
        if (cl <= i) sP[pk(i, cl)] = ld(RD, (size_t)i * n + cl);
    __syncthreads();
    double load = a.reg_dark;
    if (a.reg_mode == APV_REG_REL) load = a.reg_dark * norm2_packed(sP, n, sLam, sE, sD, sU, sMisc, tid);
    if (tid < n) sP[pk(tid, tid)] = c2(sP[pk(tid, tid)].x + load, 0.0);
    __syncthreads();
    for (int kk = 0; kk < n; ++kk) {
        const double dkk = sP[pk(kk, kk)].x;                      // uniform
        if (!(dkk > 0.0) || !(dkk < 1e300)) { status = 1; break; }
        const double sq = sqrt(dkk), inv = 1.0 / sq;
        for (int i = kk + 1 + tid; i < n; i += TPB) sP[pk(i, kk)] = cscale(sP[pk(i, kk)], inv);
        if (tid == 0) sCs[kk] = sq;
        __syncthreads();
        const int j = kk + 1 + cl;
        const double2 ljk = j < n ? sP[pk(j, kk)] : c2(0, 0);
        for (int i = kk + 1 + rg; i < n; i += 8)
            if (j <= i) sP[pk(i, j)] = csub(sP[pk(i, j)], cmulc(sP[pk(i, kk)], ljk));
        __syncthreads();
    }
    if (status == 0) {
        // park L (column-packed, diagonal from sCs, which keeps it)
        for (int i = rg; i < n; i += 8)
            if (cl <= i) gL[colofs(n, cl) + i - cl] = cl == i ? c2(sCs[i], 0.0) : sP[pk(i, cl)];
        __syncthreads();

        // ---------------- stage 2: R_B, bright loading, C = L^-1 R_B L^-H ----------------
        for (int i = rg; i < n; i += 8)
            if (cl <= i) sP[pk(i, cl)] = ld(RB, (size_t)i * n + cl);
        __syncthreads();
        if (a.reg_bright != 0.0) {
            const double lb = a.reg_bright * norm2_packed(sP, n, sLam, sE, sD, sU, sMisc, tid);
            if (tid < n) sP[pk(tid, tid)] = c2(sP[pk(tid, tid)].x + lb, 0.0);
            __syncthreads();
        }
        for (int kk = 0; kk < n; ++kk) {
            // column kk of L -> sLc (diagonal included)
            if (tid < n - kk) sLc[kk + tid] = gL[colofs(n, kk) + tid];
            __syncthreads();
            const double lkk = sLc[kk].x;
            const double akk = sP[pk(kk, kk)].x / (lkk * lkk);
            const double ct = -0.5 * akk;
            const int i1 = kk + 1 + tid;
            if (i1 < n) sU[i1] = cadd(cscale(sP[pk(i1, kk)], 1.0 / lkk), cscale(sLc[i1], ct));
            __syncthreads();
            const int j = kk + 1 + cl;
            if (j < n) {
                const double2 uj = sU[j], lj = sLc[j];
                for (int i = kk + 1 + rg; i < n; i += 8) {
                    if (j > i) continue;
                    const double2 ui = sU[i], li = sLc[i];
                    double2 v = csub(sP[pk(i, j)], cadd(cmulc(ui, lj), cmulc(li, uj)));
                    if (i == j) v.y = 0.0;
                    sP[pk(i, j)] = v;
                }
            }
            if (i1 < n) sP[pk(i1, kk)] = cadd(sU[i1], cscale(sLc[i1], ct));
            if (tid == 0) sP[pk(kk, kk)] = c2(akk, 0.0);
            __syncthreads();
        }
        // the deferred solves, column k below the diagonal <- L[k+1:, k+1:]^-1 x, by forward substitution over the rows (triangular
        // solves, not products with an explicit inverse: those lose cond(L) digits when R_D is nearly singular); column lane 127
        // carries r~ = L^-1 r along (l from 0).  Row i reads rows l < i only.
        for (int i = 0; i < n; ++i) {
            const bool rcol = cl == NM - 1;
            const int kc = rcol ? -1 : cl;
            double2 s = c2(0, 0);
            if (rcol || cl < i)
                for (int l = kc + 1 + rg; l < i; l += 8) {
                    const double2 lil = gL[colofs(n, l) + i - l];
                    s = cadd(s, cmul(lil, rcol ? sR[l] : sP[pk(l, kc)]));
                }
            sRed[rg * NM + cl] = s;
            __syncthreads();
            if (tid < NM && (tid == NM - 1 || tid < i)) {
                double2 t = c2(0, 0);
                for (int g = 0; g < 8; ++g) t = cadd(t, sRed[g * NM + tid]);
                const double il = 1.0 / sCs[i];
                if (tid == NM - 1) sR[i] = cscale(csub(sR[i], t), il);
                else sP[pk(i, tid)] = cscale(csub(sP[pk(i, tid)], t), il);
            }
            __syncthreads();
        }

        // ---------------- stage 3: Householder tridiagonalisation (zhetd2, lower), y = Q^H r~ ----------------
        for (int i = 0; i + 1 < n; ++i) {
            const int l0 = i + 2 + tid;
            const double xs = (tid < 128 && l0 < n) ? cabs2(sP[pk(l0, i)]) : 0.0;
            const double xnorm2 = sum128(xs, sScal, tid);
            const double2 alpha = sP[pk(i + 1, i)];
            double2 tau = c2(0, 0), scale = c2(0, 0);
            double e_i = alpha.x;
            const bool refl = !(xnorm2 == 0.0 && alpha.y == 0.0);
            if (refl) {
                const double beta = -copysign(sqrt(alpha.x * alpha.x + alpha.y * alpha.y + xnorm2), alpha.x);
                tau = c2((beta - alpha.x) / beta, -alpha.y / beta);
                const double2 dn = c2(alpha.x - beta, alpha.y);           // 1 / (alpha - beta)
                const double id = 1.0 / cabs2(dn);
                scale = c2(dn.x * id, -dn.y * id);
                e_i = beta;
            }
            if (tid == 0) {
                sD[i] = sP[pk(i, i)].x;
                sE[i] = e_i;
                sTau[i] = tau;
            }
            if (!refl) {                                                   // uniform
                if (tid == 0) sP[pk(i + 1, i + 1)].y = 0.0;
                __syncthreads();
                continue;
            }
            // v = [1; x * scale] over rows i+1..n-1 -> sU, and back into column i
            if (tid < n - i - 1) {
                const int l = i + 1 + tid;
                double2 v = c2(1.0, 0.0);
                if (l > i + 1) {
                    v = cmul(sP[pk(l, i)], scale);
                    sP[pk(l, i)] = v;
                }
                sU[l] = v;
            }
            __syncthreads();
            // x = tau A22 v, partial sums over columns l = i+1+rg (mod 8)
            {
                const int jr = i + 1 + cl;
                double2 s = c2(0, 0);
                if (jr < n)
                    for (int l = i + 1 + rg; l < n; l += 8) {
                        const double2 h = (l <= jr) ? sP[pk(jr, l)] : cconj(sP[pk(l, jr)]);
                        s = cadd(s, cmul(h, sU[l]));
                    }
                sRed[rg * NM + cl] = s;
            }
            __syncthreads();
            double2 xv = c2(0, 0);
            const int jr = i + 1 + tid;
            if (tid < 128 && jr < n) {
                double2 t = c2(0, 0);
                for (int g = 0; g < 8; ++g) t = cadd(t, sRed[g * NM + tid]);
                xv = cmul(tau, t);
            }
            // alpha2 = -1/2 tau (x^H v)
            const double2 vj = (tid < 128 && jr < n) ? sU[jr] : c2(0, 0);
            const double2 pr = ccmul(xv, vj);
            const double dre = sum128(pr.x, sScal, tid);
            const double dim = sum128(pr.y, sScal, tid);
            const double2 a2 = cscale(cmul(tau, c2(dre, dim)), -0.5);
            if (tid < 128 && jr < n) sLc[jr] = cadd(xv, cmul(a2, vj));
            __syncthreads();
            // A22 -= v x^H + x v^H
            {
                const int j = i + 1 + cl;
                if (j < n) {
                    const double2 vjj = sU[j], xj = sLc[j];
                    for (int r = i + 1 + rg; r < n; r += 8) {
                        if (j > r) continue;
                        double2 v = csub(sP[pk(r, j)], cadd(cmulc(sU[r], xj), cmulc(sLc[r], vjj)));
                        if (r == j) v.y = 0.0;
                        sP[pk(r, j)] = v;
                    }
                }
            }
            __syncthreads();
            // y <- H_i^H y = y - conj(tau) v (v^H y)
            const double2 py = (tid < 128 && jr < n) ? ccmul(vj, sR[jr]) : c2(0, 0);
            const double yre = sum128(py.x, sScal, tid);
            const double yim = sum128(py.y, sScal, tid);
            const double2 f = cmul(cconj(tau), c2(yre, yim));
            if (tid < 128 && jr < n) sR[jr] = csub(sR[jr], cmul(f, vj));
            __syncthreads();
        }
        if (tid == 0) {
            sD[n - 1] = sP[pk(n - 1, n - 1)].x;
            sE[n - 1] = 0.0;
        }
        // park the reflectors (column i holds v_i at rows i+2.., v_i[i+1] = 1)
        for (int r = rg; r < n; r += 8)
            if (cl + 1 < r) gV[colofs(n, cl) + r - cl] = sP[pk(r, cl)];
        __syncthreads();

        // ---------------- stage 4: implicit QL on T, Z accumulated in LDS ----------------
        for (int idx = tid; idx < n * NM; idx += TPB) {
            const int r = idx >> 7, c = idx & 127;
            sZ[idx] = (r == c) ? 1.0 : 0.0;
        }
        __syncthreads();
        // thread 0 runs the scalar recurrence (d, e in LDS) and publishes each QL step's rotations: sMisc[0] = 1 (done) or 0,
        // sMisc[1..2] = the rotated index range [lo, hi), sMisc[3] = 1 when the iteration cap was met
        int l = 0, total = 0;
        while (true) {
            if (tid == 0) {
                int done = 0, lo = 0, hi = 0, cap = 0;
                while (true) {
                    if (l >= n) { done = 1; break; }
                    int m = l;
                    for (; m < n - 1; ++m) {
                        const double dd = fabs(sD[m]) + fabs(sD[m + 1]);
                        if (fabs(sE[m]) <= 1.1102230246251565e-16 * dd) break;
                    }
                    if (m == l) { ++l; continue; }
                    if (++total > 30 * n) { done = 1; cap = 1; break; }
                    double g = (sD[l + 1] - sD[l]) / (2.0 * sE[l]);
                    double r = hypot(g, 1.0);
                    g = sD[m] - sD[l] + sE[l] / (g + copysign(r, g));
                    double s = 1.0, c = 1.0, p = 0.0;
                    int i = m - 1;
                    bool early = false;
                    for (; i >= l; --i) {
                        const double f = s * sE[i], b = c * sE[i];
                        r = hypot(f, g);
                        sE[i + 1] = r;
                        if (r == 0.0) {
                            sD[i + 1] -= p;
                            sE[m] = 0.0;
                            early = true;
                            break;
                        }
                        s = f / r;
                        c = g / r;
                        g = sD[i + 1] - p;
                        r = (sD[i] - g) * s + 2.0 * c * b;
                        p = s * r;
                        sD[i + 1] = g + p;
                        g = c * r - b;
                        sCs[i] = c;
                        sSn[i] = s;
                    }
                    lo = early ? i + 1 : l;
                    hi = m;
                    if (!early) {
                        sD[l] -= p;
                        sE[l] = g;
                        sE[m] = 0.0;
                    }
                    if (hi > lo) break;                // rotations to apply
                }
                sMisc[0] = done;
                sMisc[1] = lo;
                sMisc[2] = hi;
                sMisc[3] = cap;
            }
            __syncthreads();
            const int done = sMisc[0], lo = sMisc[1], hi = sMisc[2];
            if (done) {
                if (sMisc[3]) status = 2;
                break;
            }
            if (tid < n) {
                double* zr = sZ + tid * NM;
                double zi1 = zr[hi];
                for (int i = hi - 1; i >= lo; --i) {
                    const double c = sCs[i], s = sSn[i], zi = zr[i];
                    zr[i + 1] = s * zi + c * zi1;
                    zi1 = c * zi - s * zi1;
                }
                zr[lo] = zi1;
            }
            __syncthreads();
        }

        // ---------------- stage 5: order, coefficients ----------------
        if (tid < n) {
            const double li = sD[tid];
            int rank = 0;
            for (int j = 0; j < n; ++j) {
                const double lj = sD[j];
                rank += (lj > li) || (lj == li && j < tid);
            }
            sOrd[rank] = tid;
            double2 c = c2(0, 0);
            for (int r = 0; r < n; ++r) c = cadd(c, cscale(sR[r], sZ[r * NM + tid]));
            sU[tid] = cscale(c, 1.0 / (li + span_mu<SPAN, double>(a.span, z == 1, k, a.mu)));
        }
        __syncthreads();
        if (tid < n) sLam[tid] = sD[sOrd[tid]];
        __syncthreads();
    }

    // ---------------- stage 6: outputs ----------------
    const bool ok = status != 1;
    if (tid < n && a.lam[z]) {
        const double lv = ok ? sLam[tid] : 0.0;
        if (a.out_c128) reinterpret_cast<double*>(a.lam[z])[(size_t)k * n + tid] = lv;
        else reinterpret_cast<float*>(a.lam[z])[(size_t)k * n + tid] = (float)lv;
    }
    if (tid == 0 && a.status[z]) a.status[z][k] = status;
    // columns in groups of 8: the nV filters, then (U requested) the n eigenvectors.  col < nV: s_V; else z of rank col - nV
    const int ncols = a.nV + ((a.U && z == 0) ? n : 0);
    // the span of the bin (gevd_span.h): no slot goes past s_k; n without a span.  (sD, sU: by unsorted column, like sOrd's entries)
    const int s_k = span_limit<SPAN, double>(a.span, z == 1, k, n, a.ranks[a.nV - 1], ok, true, sD, sU, sOrd, tid);
    for (int c0 = 0; c0 < ncols; c0 += 8) {
        const int col = c0 + rg;
        const bool live = col < ncols && cl < n;
        double2 y = c2(0, 0);
        if (ok && live) {
            if (col < a.nV) {
                const int V = SPAN ? min(a.ranks[col], s_k) : a.ranks[col];
                for (int t = 0; t < V; ++t) {
                    const int q = sOrd[t];
                    y = cadd(y, cscale(sU[q], sZ[cl * NM + q]));
                }
            } else {
                y = c2(sZ[cl * NM + sOrd[col - a.nV]], 0.0);
            }
        }
        if (ok) {
            // y <- Q y = H_0 (H_1 (... H_{n-2} y)), H_i = I - tau_i v_i v_i^H
            for (int i = n - 2; i >= 0; --i) {
                const double2 tau = sTau[i];
                if (tau.x == 0.0 && tau.y == 0.0) continue;      // uniform
                double2 v = c2(0, 0);
                if (cl == i + 1) v = c2(1.0, 0.0);
                else if (cl > i + 1 && cl < n) v = gV[colofs(n, i) + cl - i];
                const double2 pr = ccmul(v, y);                   // v^H y, per column
                double px = pr.x, py = pr.y;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    px += __shfl_xor(px, off);
                    py += __shfl_xor(py, off);
                }
                // per column group rg: waves 2 rg and 2 rg + 1 (the barrier at the end of the previous reflector freed sLc)
                if ((tid & 63) == 0) sLc[tid >> 6] = c2(px, py);
                __syncthreads();
                const double2 dv = cadd(sLc[2 * rg], sLc[2 * rg + 1]);
                y = csub(y, cmul(cmul(tau, dv), v));
                __syncthreads();
            }
            sRed[rg * NM + cl] = y;
        }
        __syncthreads();
        // x = L^-H y by back substitution, in place in sRed: x_i = (y_i - sum_{l > i} conj(L_li) x_l) / L_ii
        if (ok) {
            for (int i = n - 1; i >= 0; --i) {
                double2 pr = c2(0, 0);
                if (cl > i && cl < n) pr = ccmul(gL[colofs(n, i) + cl - i], sRed[rg * NM + cl]);
                double px = pr.x, py = pr.y;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    px += __shfl_xor(px, off);
                    py += __shfl_xor(py, off);
                }
                if ((tid & 63) == 0) sLc[tid >> 6] = c2(px, py);
                __syncthreads();
                if (cl == i) {
                    const double2 t = cadd(sLc[2 * rg], sLc[2 * rg + 1]);
                    sRed[rg * NM + i] = cscale(csub(sRed[rg * NM + i], t), 1.0 / gL[colofs(n, i)].x);   // (sCs holds QL's c now)
                }
                __syncthreads();
            }
        }
        const double2 x = (ok && live) ? sRed[rg * NM + cl] : c2(0, 0);
        if (live) {
            if (col < a.nV) {
                const size_t o = ((size_t)k * a.nV + col) * n + cl;
                if (a.out_c128) reinterpret_cast<double2*>(a.w[z])[o] = x;
                else reinterpret_cast<float2*>(a.w[z])[o] = make_float2((float)x.x, (float)x.y);
            } else {
                st(reinterpret_cast<RT*>(a.U), ((size_t)k * n + cl) * n + (col - a.nV), x);
            }
        }
        __syncthreads();
    }
}

std::atomic<unsigned long long> g_attr_c64{0}, g_attr_c128{0}, g_attr_span_c64{0}, g_attr_span_c128{0};

}  // namespace

size_t apv_gevd128_slot_bytes(int n) { return (2 * (size_t)n * n + n) * 16; }

hipError_t apv_launch_corr128(int K, int M, int L, int x_c128, const void* XB, const void* XD, const void* d, double2* RB,
                              double2* RD, double2* r, hipStream_t s) {
    if (L < 1 || L > NM || M < 1 || K < 0) return hipErrorInvalidValue;
    if (K == 0) return hipSuccess;
    Corr128Args a{};
    a.K = K; a.M = M; a.n = L;
    const int T = (L + CT - 1) / CT;
    a.n_tiles = T * (T + 1) / 2;
    a.XB[0] = XB; a.XD[0] = XD; a.d[0] = d;
    a.RB = RB; a.RD = RD; a.rr = r;
    const dim3 grid(2 * a.n_tiles, K, 1);
    if (x_c128) hipLaunchKernelGGL(corr128_kernel<double2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(corr128_kernel<float2>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t apv_launch_gevd128(const GevdParams& p, int compute_dtype, bool fused, hipStream_t s, std::string* why,
                              const int32_t* ranks_all) {
    const int n = p.n;
    if (n <= APV_MAX_N || n > APV_MAX_SRCS) {
        if (why) *why = "GEVD order n out of range (65..128 for this kernel)";
        return hipErrorInvalidValue;
    }
    if (p.x_group > 1) {
        if (why) *why = "grouped spectra (x_group > 1) are read by the order-16 float64 kernel only";
        return hipErrorInvalidValue;
    }
    if (p.n_hops > 1) {
        if (why) *why = "several hops per launch (n_hops > 1) are taken by the order-16 kernels on fused slabs only";
        return hipErrorInvalidValue;
    }
    if (p.nV < 1 || p.nV > n || (p.nV > APV_MAX_RANKS && ranks_all == nullptr)) {
        if (why) *why = "rank list out of range";
        return hipErrorInvalidValue;
    }
    if (p.Lspill == nullptr) {
        if (why) *why = "orders 65..128 need the per-bin scratch (apv_gevd_spill_bytes)";
        return hipErrorInvalidValue;
    }
    if (p.K <= 0) return hipSuccess;
    const int zones = (fused && p.n_zones > 1) ? 2 : 1;
    Gevd128Args a{};
    a.n = n; a.K = p.K; a.nV = p.nV;
    a.reg_mode = p.reg_mode; a.out_c128 = p.out_c128;
    a.reg_dark = p.reg_dark; a.reg_bright = p.reg_bright; a.mu = p.mu;
    a.span = p.span;
    for (int t = 0; t < p.nV; ++t) {
        const int V = ranks_all ? ranks_all[t] : p.ranks[t];
        if (V < 1 || V > n) {
            if (why) *why = "rank V out of 1..L";
            return hipErrorInvalidValue;
        }
        a.ranks[t] = V;
    }
    double2* const slot = reinterpret_cast<double2*>(p.Lspill);
    const size_t sl = apv_gevd128_slot_bytes(n) / 16;
    a.slot = slot;
    a.w[0] = p.w; a.lam[0] = p.lam; a.status[0] = p.status;
    a.w[1] = p.w1; a.lam[1] = p.lam1; a.status[1] = p.status1;
    a.U = fused ? nullptr : p.U;
    bool in64 = false;
    if (fused) {
        // stage 0 into the slots, then the solve from them (c128)
        Corr128Args c{};
        c.K = p.K; c.M = p.M; c.n = n;
        const int T = (n + CT - 1) / CT;
        c.n_tiles = T * (T + 1) / 2;
        c.XB[0] = p.XB; c.XD[0] = p.XD; c.d[0] = p.d;
        c.XB[1] = p.XB1; c.XD[1] = p.XD1; c.d[1] = p.d1;
        c.out = slot;
        c.slot = sl;
        const dim3 cg(2 * c.n_tiles, p.K, zones);
        if (p.x_c128) hipLaunchKernelGGL(corr128_kernel<double2>, cg, dim3(256), 0, s, c);
        else hipLaunchKernelGGL(corr128_kernel<float2>, cg, dim3(256), 0, s, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        for (int zz = 0; zz < zones; ++zz) {
            double2* base = slot + (size_t)zz * p.K * sl;
            a.RB[zz] = base;
            a.RD[zz] = base + (size_t)n * n;
            a.r[zz] = base + 2 * (size_t)n * n;
        }
        a.in_mat = sl;
        a.in_vec = sl;
    } else {
        a.RB[0] = p.RB; a.RD[0] = p.RD; a.r[0] = p.r;
        a.in_mat = (size_t)n * n;
        a.in_vec = n;
        in64 = compute_dtype != APV_F64;
    }
    const dim3 grid(p.K, zones);
    // one instantiation per (input type, span or none), each with its own record of the LDS attribute
    auto launch = [&](auto kernel, std::atomic<unsigned long long>& done) -> hipError_t {
        const hipError_t e = apv_set_max_dynamic_lds(reinterpret_cast<const void*>(kernel), LDS_BYTES, done);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, grid, dim3(TPB), LDS_BYTES, s, a);
        return hipGetLastError();
    };
    if (p.span.on) return in64 ? launch(&gevd128_kernel<float2, true>, g_attr_span_c64) : launch(&gevd128_kernel<double2, true>, g_attr_span_c128);
    return in64 ? launch(&gevd128_kernel<float2, false>, g_attr_c64) : launch(&gevd128_kernel<double2, false>, g_attr_c128);
}
