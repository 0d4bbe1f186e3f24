// Spectral norms of up to four symmetric positive semi-definite matrices (apv_launch_norm2): the relative loading of the
// broadband stream and of the large joint diagonalisation (capi.hip, kernels_jdiag_cplx.hip, stream_bb.hip).
#include "apv_internal.h"

namespace {

// lambda_max of a symmetric positive semi-definite n x n matrix (= norm(R), apVast.m:559-566): KL Lanczos steps and
// the largest eigenvalue of the resulting tridiagonal matrix by 1024-way multisection on Sturm counts.  One workgroup
// per matrix; in the matrix-vector product a wave takes a row at a time so that the loads run along it.  (Plain power
// iteration needs thousands of steps when the leading eigenvalues cluster, which they do right after start-up.)
constexpr int KL = 96;
struct NormJobs {
    const double* m[4];
};

// The largest eigenvalue of the k x k tridiagonal matrix (alpha, beta[1..k)) by seven rounds of 1024-way multisection on
// Sturm counts from its Gershgorin bracket; every thread of a 1024-thread workgroup returns it.  red [32], flag [1025]: LDS.
__device__ __forceinline__ double tridiag_max_eig(const double* alpha, const double* beta, int k, double* red, int* flag, int tid,
                                                  int wave, int lane) {
    // Gershgorin bracket of the tridiagonal matrix, then multisection: count(x) = number of eigenvalues below x
    double lo = alpha[0], hi = alpha[0];
    for (int i = 0; i < k; ++i) {
        const double rad = (i > 0 ? fabs(beta[i]) : 0.0) + (i + 1 < k ? fabs(beta[i + 1]) : 0.0);
        lo = fmin(lo, alpha[i] - rad);
        hi = fmax(hi, alpha[i] + rad);
    }
    for (int round = 0; round < 7; ++round) {
        const double x = lo + (hi - lo) * (double)(tid + 1) / 1025.0;
        int cnt = 0;
        double dd = 1.0;
        for (int i = 0; i < k; ++i) {
            const double b2 = i > 0 ? beta[i] * beta[i] : 0.0;
            dd = (alpha[i] - x) - (i > 0 ? b2 / dd : 0.0);
            if (dd == 0.0) dd = -1e-300;
            cnt += dd < 0.0;
        }
        flag[tid + 1] = cnt >= k;                  // every eigenvalue lies below x
        if (tid == 0) flag[0] = 0;
        __syncthreads();
        // the largest eigenvalue sits between the last x that is not above all of them and the first that is
        const double step = (hi - lo) / 1025.0;
        double nlo = lo, nhi = hi;
        int first = 1025;
        for (int q = wave * 64 + lane; q < 1024; q += 1024) first = (flag[q + 1] && !flag[q]) ? q : first;
        // reduce `first` (exactly one boundary exists since the counts are monotone)
        red[0] = 0;
        __syncthreads();
        if (first < 1025) {
            red[0] = (double)first;
            red[1] = 1.0;
        }
        if (tid == 0 && !flag[1024]) red[1] = 0.0;
        __syncthreads();
        if (flag[1024]) {
            const int f = (int)red[0];
            nlo = lo + step * (double)f;
            nhi = lo + step * (double)(f + 1);
        } else {
            nlo = lo + step * 1024.0;              // numerically above the bracket: keep the top slice
        }
        __syncthreads();
        lo = nlo;
        hi = nhi;
    }
    return 0.5 * (lo + hi);
}

__global__ void __launch_bounds__(1024) norm2_lanczos_kernel(int n, NormJobs jobs, double* __restrict__ out) {
    extern __shared__ double pw[];               // v [n], vp [n], w [n], alpha [KL], beta [KL + 1], red [32], flag [1025]
    const double* __restrict__ Rm = jobs.m[blockIdx.x];
    double *v = pw, *vp = pw + n, *w = pw + 2 * n, *alpha = pw + 3 * n, *beta = alpha + KL, *red = beta + KL + 1;
    int* flag = reinterpret_cast<int*>(red + 32);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    auto block_sum = [&](double a) {             // sum over the workgroup, result in every thread
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        __syncthreads();
        if (lane == 0) red[wave] = a;
        __syncthreads();
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += red[q];
        return t;
    };
    double nrm0 = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const double x = 1.0 + 0.37 * (double)((i * 7) % 11);
        v[i] = x;
        vp[i] = 0.0;
        nrm0 += x * x;
    }
    nrm0 = block_sum(nrm0);
    const double inv0 = 1.0 / sqrt(nrm0);
    for (int i = tid; i < n; i += 1024) v[i] *= inv0;
    if (tid == 0) beta[0] = 0.0;
    __syncthreads();
    const int kmax = n < KL ? n : KL;
    int k = 0;
    for (int j = 0; j < kmax; ++j) {
        for (int row = wave; row < n; row += 16) {
            double a = 0.0;
            for (int c = lane; c < n; c += 64) a += Rm[(size_t)row * n + c] * v[c];
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
            if (lane == 0) w[row] = a;
        }
        __syncthreads();
        double d = 0.0;
        for (int i = tid; i < n; i += 1024) d += v[i] * w[i];
        const double aj = block_sum(d);
        const double bj = beta[j];
        double nn2 = 0.0;
        for (int i = tid; i < n; i += 1024) {
            const double x = w[i] - aj * v[i] - bj * vp[i];
            w[i] = x;
            nn2 += x * x;
        }
        nn2 = block_sum(nn2);
        const double bn = sqrt(nn2);
        if (tid == 0) {
            alpha[j] = aj;
            beta[j + 1] = bn;
        }
        k = j + 1;
        if (!(bn > 1e-14 * fabs(aj)) || !(bn > 1e-300)) break;          // invariant subspace found (uniform)
        const double ib = 1.0 / bn;
        for (int i = tid; i < n; i += 1024) {
            vp[i] = v[i];
            v[i] = w[i] * ib;
        }
        __syncthreads();
    }
    __syncthreads();
    const double top = tridiag_max_eig(alpha, beta, k, red, flag, tid, wave, lane);
    if (tid == 0) out[blockIdx.x] = top;
}

// The same KL Lanczos steps from the same start vector for large orders, with the matrix-vector product of each step spread
// over the chip: one launch per step (no communication between workgroups inside a launch).  Launch s (grid: row blocks x
// matrices) first finishes step s - 1 in EVERY workgroup -- alpha = v.w, x = w - alpha v - beta vp, beta' = |x|, v' = x / beta'
// -- which is n-long work done redundantly, so each workgroup holds the new vector with no hand-off; the same code on the
// same data gives the same bits in all of them.  Workgroup 0 stores v' and the scalars, then every workgroup multiplies its
// NG_ROWS rows by v'.  Launch 0 starts from the normalised start vector.  A last launch runs the multisection.
constexpr int NG_TPB = 512, NG_ROWS = 32;               // 8 waves, 4 rows each
// workspace per matrix, in doubles: V [3][n] (ring: step s writes slot s % 3), W [2][n] (R v of step s in slot s % 2), then
// alpha [KL], beta [KL + 1], stop [KL + 1] (set once step s has stopped), k
__host__ __device__ inline size_t norm2_ws_stride(int n) { return 5 * (size_t)n + 3 * KL + 3; }

__global__ void __launch_bounds__(NG_TPB) norm2_grid_step_kernel(int n, int s, NormJobs jobs, double* __restrict__ ws) {
    extern __shared__ double xv[];                       // [n] the step's Lanczos vector
    __shared__ double red[NG_TPB / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int q = blockIdx.y;
    double* const base = ws + (size_t)q * norm2_ws_stride(n);
    double *V = base, *Wv = base + 3 * (size_t)n, *alpha = base + 5 * (size_t)n, *beta = alpha + KL, *stop = beta + KL + 1,
           *kout = stop + KL + 1;
    const bool lead = blockIdx.x == 0 && tid == 0;
    auto block_sum = [&](double a) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        __syncthreads();
        if (lane == 0) red[wave] = a;
        __syncthreads();
        double t = 0.0;
        for (int w = 0; w < NG_TPB / 64; ++w) t += red[w];
        return t;
    };
    const int kmax = n < KL ? n : KL;
    if (s == 0) {
        double nrm0 = 0.0;
        for (int i = tid; i < n; i += NG_TPB) {
            const double x = 1.0 + 0.37 * (double)((i * 7) % 11);
            xv[i] = x;
            nrm0 += x * x;
        }
        const double inv0 = 1.0 / sqrt(block_sum(nrm0));
        for (int i = tid; i < n; i += NG_TPB) xv[i] *= inv0;
        if (lead) {
            beta[0] = 0.0;
            stop[0] = 0.0;
            kout[0] = 0.0;
        }
    } else {
        if (stop[s - 1] != 0.0) {                        // an earlier step found an invariant subspace (uniform)
            if (lead) stop[s] = 1.0;
            return;
        }
        const double* v = V + (size_t)((s - 1) % 3) * n;
        const double* vp = V + (size_t)((s + 1) % 3) * n;        // slot (s - 2) % 3; not read at s = 1
        const double* w = Wv + (size_t)((s - 1) % 2) * n;
        double d = 0.0;
        for (int i = tid; i < n; i += NG_TPB) d += v[i] * w[i];
        const double aj = block_sum(d);
        const double bj = beta[s - 1];
        double nn2 = 0.0;
        for (int i = tid; i < n; i += NG_TPB) {
            const double x = w[i] - aj * v[i] - (s > 1 ? bj * vp[i] : 0.0);
            xv[i] = x;
            nn2 += x * x;
        }
        nn2 = block_sum(nn2);
        const double bn = sqrt(nn2);
        const bool done = !(bn > 1e-14 * fabs(aj)) || !(bn > 1e-300) || s == kmax;
        if (lead) {
            alpha[s - 1] = aj;
            beta[s] = bn;
            kout[0] = (double)s;
            stop[s] = done ? 1.0 : 0.0;
        }
        if (done) return;
        const double ib = 1.0 / bn;
        for (int i = tid; i < n; i += NG_TPB) xv[i] *= ib;
    }
    if (blockIdx.x == 0)
        for (int i = tid; i < n; i += NG_TPB) V[(size_t)(s % 3) * n + i] = xv[i];
    __syncthreads();
    // w = R v on this workgroup's rows: a wave takes four rows at once, so that four loads along them are in flight per lane
    const double* __restrict__ Rm = jobs.m[q];
    const int r0 = blockIdx.x * NG_ROWS + wave * 4;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (r0 + 3 < n) {
        const double* p = Rm + (size_t)r0 * n;
#pragma unroll 2
        for (int c = lane; c < n; c += 64) {
            const double x = xv[c];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] += p[(size_t)u * n + c] * x;
        }
    } else {
        for (int u = 0; u < 4 && r0 + u < n; ++u) {
            const double* p = Rm + (size_t)(r0 + u) * n;
            for (int c = lane; c < n; c += 64) a[u] += p[c] * xv[c];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) a[u] += __shfl_xor(a[u], o, 64);
        if (lane == 0 && r0 + u < n) Wv[(size_t)(s % 2) * n + r0 + u] = a[u];
    }
}

// the multisection of norm2_lanczos_kernel on the tridiagonal matrices the steps left behind, one workgroup per matrix
__global__ void __launch_bounds__(1024) norm2_grid_finish_kernel(int n, const double* __restrict__ ws, double* __restrict__ out) {
    __shared__ double ab[2 * KL + 1 + 32];
    __shared__ int flag[1025];
    const double* base = ws + (size_t)blockIdx.x * norm2_ws_stride(n);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *alpha = ab, *beta = ab + KL, *red = ab + 2 * KL + 1;
    for (int i = tid; i < 2 * KL + 1; i += 1024) ab[i] = base[5 * (size_t)n + i];
    const int k = (int)base[5 * (size_t)n + 3 * KL + 2];
    __syncthreads();
    const double top = tridiag_max_eig(alpha, beta, k, red, flag, tid, wave, lane);
    if (tid == 0) out[blockIdx.x] = top;
}

}  // namespace

hipError_t apv_launch_norm2(int n, int count, const double* const* d_mats, double* d_out, hipStream_t s, int method) {
    if (count < 1 || count > 4 || n < 1 || n > APV_NORM2_MAX_N) return hipErrorInvalidValue;
    NormJobs nj{};
    for (int q = 0; q < count; ++q) nj.m[q] = d_mats[q];
    if (method == APV_NORM2_AUTO) method = n > APV_NORM2_GRID_MIN_N ? APV_NORM2_GRID : APV_NORM2_ONE_WG;
    if (method == APV_NORM2_ONE_WG) {
        const size_t lds = sizeof(double) * (3 * (size_t)n + 2 * KL + 33 + 520);
        if (lds > 64 * 1024) {                     // n > 2482
            static std::atomic<unsigned long long> attr_set{0};
            const hipError_t e = apv_set_max_dynamic_lds(reinterpret_cast<const void*>(&norm2_lanczos_kernel),
                                                         (int)(sizeof(double) * (3 * APV_NORM2_MAX_N + 2 * KL + 33 + 520)), attr_set);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(norm2_lanczos_kernel, dim3(count), dim3(1024), lds, s, n, nj, d_out);
        return hipGetLastError();
    }
    if (method != APV_NORM2_GRID) return hipErrorInvalidValue;
    // the workspace is the stream's: concurrent calls on other streams each have their own
    double* ws = nullptr;
    hipError_t e = hipMallocAsync((void**)&ws, sizeof(double) * norm2_ws_stride(n) * count, s);
    if (e != hipSuccess) return e;
    const int kmax = n < KL ? n : KL;
    const dim3 grid((n + NG_ROWS - 1) / NG_ROWS, count);
    for (int step = 0; step <= kmax; ++step) {
        hipLaunchKernelGGL(norm2_grid_step_kernel, grid, dim3(NG_TPB), sizeof(double) * (size_t)n, s, n, step, nj, ws);
        if ((e = hipGetLastError()) != hipSuccess) break;
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(norm2_grid_finish_kernel, dim3(count), dim3(1024), 0, s, n, (const double*)ws, d_out);
        e = hipGetLastError();
    }
    const hipError_t fe = hipFreeAsync(ws, s);
    return e != hipSuccess ? e : fe;
}
