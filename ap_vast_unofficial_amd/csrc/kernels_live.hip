// Responses and mu reassigned between two hops (apv_stream_set_rirs / apv_bb_set_rirs).
//
// The reference filters every hop with lfilter(rir, 1, x, zi=state) (apvast.py:167-193) and reads self.rir_* on every hop: after
// `ap.rir_A = new`, each sample that arrived before the update keeps ringing out through the response it was filtered with (zi holds
// that tail), the samples from the update on go through the new one.  The device keeps input histories, not zi: K1 computes the new
// response over the whole history, and the difference is a finite CORRECTION TAIL per channel whose response changed from b to b'
// (delta = b - b'):
//     c[n][ch] = sum_{j = n+1}^{P-1} delta[j][ch] x[n - j],   n = 0 .. P-2     (x[-1] = newest sample before the update)
// It is added to K1's output of the next ceil((P-1)/H) hops.  Tails compose additively: a second update while a tail is still
// draining adds its own tail, over the full history, to what is left of the first.
//
//   fir_tail_kernel   : the tails of every changed channel in one launch (job table), float64 on v_mfma_f64_16x16x4_f64
//   tail_apply_kernel : add the next n samples of every live tail to K1's output, then shift the tail (emptied in place)
#include "apv_internal.h"

#include <algorithm>
#include <atomic>
#include <cstring>

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;

template <typename T>
struct TailJobs {
    const T* old[FIR_JOBS_D];      // [P][C_j] bank as it was (still in rir[z] / trir[z])
    const T* nw[FIR_JOBS_D];       // [P][C_j] bank that replaces it
    const T* xh[FIR_JOBS_D];       // the P - 1 newest input samples before the update, oldest first
    T* corr[FIR_JOBS_D];           // [C_j][P-1] tails, accumulated into
    int C[FIR_JOBS_D];
    int tile0[FIR_JOBS_D + 1];     // first channel tile of each job
};

// The tail is the full convolution of delta with the history continued by zeros: x~[u] = xh[u] for u < P - 1, 0 after, and
//   c[n] = sum_p delta[p] x~[P - 1 + n - p].
// A workgroup owns 16 NT samples x 16 channels, as fir_f64_mfma_kernel does for K1: the taps are the B operands (formed as
// old - new in float64 on the way in), the A operands are windows of x~ in LDS.  Taps p <= n0 only ever meet samples after the
// update, so a tile starts at tap n0 + 1 (half of the square is skipped); the taps go in blocks of TB so that the window stays
// small for any P.  The four waves split each block and their partial tiles are summed through LDS.
template <typename T, int NT>
__global__ void __launch_bounds__(256) fir_tail_kernel(int P, int njobs, TailJobs<T> jobs) {
    extern __shared__ double tail_lds[];        // [TB + 16 NT - 1] window, afterwards [4][NT][264] partial tiles
    constexpr int SB = 32;                      // k-steps (4 taps each) per wave per block
    constexpr int TB = 4 * 4 * SB;              // taps per block
    constexpr int SPAN = 16 * NT - 1;
    const int Q = P - 1;
    const int by = blockIdx.y;
    int j = 0;
    while (j + 1 < njobs && by >= jobs.tile0[j + 1]) ++j;
    const int C = jobs.C[j];
    const T* __restrict__ old = jobs.old[j];
    const T* __restrict__ nw = jobs.nw[j];
    const T* __restrict__ xh = jobs.xh[j];
    const int c0 = (by - jobs.tile0[j]) * 16, n0 = blockIdx.x * 16 * NT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, il = lane & 15, kq = lane >> 4;
    const int c = c0 + il;
    const bool c_ok = c < C;
    double* xw = tail_lds;
    d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (d4){0, 0, 0, 0};
    const int s_lo = (n0 + 1) >> 2, s_hi = (P + 3) >> 2;
    for (int sb = s_lo; sb < s_hi; sb += 4 * SB) {
        // window slot i holds x~[base + i]; base belongs to the block's last tap pmax and the tile's first sample
        const int pmax = 4 * (sb + 4 * SB) - 1;
        const int base = Q + n0 - pmax;
        __syncthreads();                         // the previous block is done with the window
        for (int i = tid; i < TB + SPAN; i += 256) {
            const int u = base + i;
            xw[i] = (u >= 0 && u < Q) ? (double)xh[u] : 0.0;
        }
        __syncthreads();
        const int w0 = sb + wave * SB, w1 = min(w0 + SB, s_hi);
        for (int st = w0; st < w1; ++st) {
            const int pt = 4 * st + kq;
            const double b = (pt < P && c_ok) ? (double)old[(size_t)pt * C + c] - (double)nw[(size_t)pt * C + c] : 0.0;
            const int wi = pmax - pt + il;       // slot of x~[Q + n0 + il - pt]
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xw[wi + 16 * t], b, acc[t], 0, 0, 0);
        }
    }
    // the four waves' partial tiles, summed as in fir_f64_mfma_kernel
    constexpr int RS = 66, TS = 4 * RS;
    double* part = tail_lds;
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(wave * NT + t) * TS + r * RS + lane] = acc[t][r];
    __syncthreads();
    const int ch = tid >> 4, qs = tid & 15;
    if (c0 + ch >= C) return;
    T* __restrict__ dst = jobs.corr[j] + (size_t)(c0 + ch) * Q;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int sm = qs * NT + u, t = sm >> 4, wi = sm & 15;
        const int e = t * TS + (wi >> 2) * RS + (wi & 3) * 16 + ch;
        const double v = part[e] + part[NT * TS + e] + part[2 * NT * TS + e] + part[3 * NT * TS + e];
        const int n = n0 + sm;
        if (n < Q) dst[n] = (T)((double)dst[n] + v);
    }
}

template <typename T>
struct TailApplyJobs {
    T* corr[FIR_JOBS_D];           // [C_j][Q]
    T* dst[FIR_JOBS_D];            // [C_j][row_len] K1 output (ring or linear buffer)
    int row0[FIR_JOBS_D + 1];      // first row (channel) of each job
};

// One workgroup per (job, channel): dst[(d0 + m) mod dmod] += corr[m] for m < n_add, then corr[m] = corr[m + shift] (zero past the
// end).  The row is walked in segments of 256 from the front: a segment's reads (m and m + shift >= m) come before its writes, and
// every later segment reads only at or behind its own start, past everything written before it.
template <typename T>
__global__ void __launch_bounds__(256) tail_apply_kernel(int Q, int n_add, int shift, long row_len, int d0, int dmod, int njobs,
                                                         TailApplyJobs<T> jobs) {
    const int row = blockIdx.x;
    int j = 0;
    while (j + 1 < njobs && row >= jobs.row0[j + 1]) ++j;
    const size_t r = (size_t)(row - jobs.row0[j]);
    T* __restrict__ cr = jobs.corr[j] + r * Q;
    T* __restrict__ dr = jobs.dst[j] + r * row_len;
    for (int m0 = 0; m0 < Q; m0 += 256) {
        const int m = m0 + (int)threadIdx.x;
        const T a = m < Q ? cr[m] : (T)0;
        const T b = m + shift < Q ? cr[m + shift] : (T)0;
        if (m < n_add && m < Q) dr[(d0 + m) % dmod] += a;
        __syncthreads();
        if (m < Q) cr[m] = b;
        __syncthreads();
    }
}

// dst[c][p] = src[p][c]: a bank in the channel-major layout the spectra of the fast-convolution K1 are formed from
template <typename T>
__global__ void __launch_bounds__(256) bank_transpose_kernel(int P, int C, const T* __restrict__ src, T* __restrict__ dst) {
    __shared__ T tile[32][33];
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (p0 + i < P && c0 + tx < C) tile[i][tx] = src[(size_t)(p0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < C && p0 + tx < P) dst[(size_t)(c0 + i) * P + p0 + tx] = tile[tx][i];
}

template <typename T>
hipError_t launch_tail(const FirLiveJobs& jb, int P, hipStream_t s) {
    TailJobs<T> jobs{};
    int tiles = 0;
    for (int j = 0; j < jb.n; ++j) {
        jobs.old[j] = (const T*)jb.old[j];
        jobs.nw[j] = (const T*)jb.nw[j];
        jobs.xh[j] = (const T*)jb.xh[j];
        jobs.corr[j] = (T*)jb.corr[j];
        jobs.C[j] = jb.C[j];
        jobs.tile0[j] = tiles;
        tiles += (jb.C[j] + 15) / 16;
    }
    jobs.tile0[jb.n] = tiles;
    if (tiles == 0 || P < 2) return hipSuccess;
    const int Q = P - 1;
    static std::atomic<unsigned long long> lds_set[2];
    if (Q >= 256) {
        constexpr int NT = 4;
        const int lds = (int)(sizeof(double) * std::max(512 + 16 * NT, 4 * NT * 264));
        hipError_t e = apv_set_max_dynamic_lds((const void*)fir_tail_kernel<T, NT>, lds, lds_set[0]);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((fir_tail_kernel<T, NT>), dim3((Q + 16 * NT - 1) / (16 * NT), tiles), dim3(256), lds, s, P, jb.n, jobs);
    } else {
        const int lds = (int)(sizeof(double) * std::max(512 + 16, 4 * 264));
        hipLaunchKernelGGL((fir_tail_kernel<T, 1>), dim3((Q + 15) / 16, tiles), dim3(256), lds, s, P, jb.n, jobs);
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_apply(const FirLiveJobs& jb, int Q, int n_add, int shift, long row_len, int d0, int dmod, hipStream_t s) {
    TailApplyJobs<T> jobs{};
    int rows = 0;
    for (int j = 0; j < jb.n; ++j) {
        jobs.corr[j] = (T*)jb.corr[j];
        jobs.dst[j] = (T*)jb.dst[j];
        jobs.row0[j] = rows;
        rows += jb.C[j];
    }
    jobs.row0[jb.n] = rows;
    if (rows == 0 || Q < 1) return hipSuccess;
    hipLaunchKernelGGL(tail_apply_kernel<T>, dim3(rows), dim3(256), 0, s, Q, n_add, shift, row_len, d0 % dmod, dmod, jb.n, jobs);
    return hipGetLastError();
}

}  // namespace

hipError_t apv_launch_fir_tail(int f64, const FirLiveJobs& jobs, int P, hipStream_t s) {
    if (jobs.n <= 0) return hipSuccess;
    if (jobs.n > FIR_JOBS_D) return hipErrorInvalidValue;
    return f64 ? launch_tail<double>(jobs, P, s) : launch_tail<float>(jobs, P, s);
}

hipError_t apv_launch_tail_apply(int f64, const FirLiveJobs& jobs, int Q, int n_add, int shift, long row_len, int d0, int dmod,
                                 hipStream_t s) {
    if (jobs.n <= 0) return hipSuccess;
    if (jobs.n > FIR_JOBS_D || dmod <= 0) return hipErrorInvalidValue;
    return f64 ? launch_apply<double>(jobs, Q, n_add, shift, row_len, d0, dmod, s)
               : launch_apply<float>(jobs, Q, n_add, shift, row_len, d0, dmod, s);
}

hipError_t apv_launch_bank_transpose(int f64, int P, int C, const void* src, void* dst, hipStream_t s) {
    const dim3 grid((P + 31) / 32, (C + 31) / 32);
    if (f64) hipLaunchKernelGGL(bank_transpose_kernel<double>, grid, dim3(256), 0, s, P, C, (const double*)src, (double*)dst);
    else hipLaunchKernelGGL(bank_transpose_kernel<float>, grid, dim3(256), 0, s, P, C, (const float*)src, (float*)dst);
    return hipGetLastError();
}

// ---- host side, shared by the subband (stream.hip) and broadband (stream_bb.hip) streams ----------------------------------------

#define LCHK(h, call)                                                                    \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess) return apv_fail(h, APV_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

void apv_live_free(FirLive& fl) {
    for (void*& b : fl.corr)
        if (b) { (void)hipFree(b); b = nullptr; }
    for (void*& b : fl.stage)
        if (b) { (void)hipFree(b); b = nullptr; }
    fl.hops_left = 0;
    for (bool& l : fl.live) l = false;
}

int apv_live_alloc(apv_handle* h, FirLive& fl, int P, int C, int M, size_t esz, hipStream_t st) {
    if (fl.corr[0]) return APV_OK;
    for (int j = 0; j < 6; ++j) {
        const size_t bytes = esz * (size_t)(j < 4 ? C : M) * (size_t)std::max(P - 1, 1);
        LCHK(h, hipMalloc(&fl.corr[j], bytes));
        LCHK(h, hipMemsetAsync(fl.corr[j], 0, bytes, st));
    }
    for (int b = 0; b < 4; ++b) LCHK(h, hipMalloc(&fl.stage[b], esz * (size_t)P * (b < 2 ? C : M)));
    return APV_OK;
}

// host (P, L, M) C order -> device [P][m L + l]; (P, M) targets are already in the device order
void apv_bank_to_device(const double* src, int P, int L, int M, bool target, std::vector<double>& out) {
    if (target) {
        out.assign(src, src + (size_t)P * M);
        return;
    }
    const size_t C = (size_t)L * M;
    out.resize((size_t)P * C);
    for (int p = 0; p < P; ++p)
        for (int l = 0; l < L; ++l)
            for (int m = 0; m < M; ++m) out[(size_t)p * C + m * L + l] = src[((size_t)p * L + l) * M + m];
}

int apv_live_update(apv_handle* h, FirLive& fl, const FirLiveBanks& b, const double* const h_new[4], hipStream_t st) {
    const int P = b.P, H = b.H, L = b.L, M = b.M, C = L * M;
    const size_t esz = b.f64 ? 8 : 4;
    int rc = apv_live_alloc(h, fl, P, C, M, esz, st);
    if (rc != APV_OK) return rc;
    // the new banks -> staging, in the front-end precision
    std::vector<double> dev;
    std::vector<float> dev32;
    for (int k = 0; k < 4; ++k) {
        if (!h_new[k]) continue;
        apv_bank_to_device(h_new[k], P, L, M, k >= 2, dev);
        if (b.f64) {
            LCHK(h, hipMemcpyAsync(fl.stage[k], dev.data(), sizeof(double) * dev.size(), hipMemcpyHostToDevice, st));
        } else {
            dev32.assign(dev.begin(), dev.end());
            LCHK(h, hipMemcpyAsync(fl.stage[k], dev32.data(), sizeof(float) * dev32.size(), hipMemcpyHostToDevice, st));
        }
        LCHK(h, hipStreamSynchronize(st));                  // dev / dev32 are rewritten for the next bank
    }
    // tails: path p takes signal p >> 1 through the bank of zone p & 1; target z takes signal z
    FirLiveJobs jobs{};
    int jid[6];
    for (int p = 0; p < 4; ++p) {
        const int z = p & 1;
        if (!h_new[z]) continue;
        jobs.old[jobs.n] = b.rir[z]; jobs.nw[jobs.n] = fl.stage[z]; jobs.xh[jobs.n] = b.hist_tail[p >> 1];
        jobs.corr[jobs.n] = fl.corr[p]; jobs.C[jobs.n] = C; jid[jobs.n++] = p;
    }
    for (int z = 0; z < 2; ++z) {
        if (!h_new[2 + z]) continue;
        jobs.old[jobs.n] = b.trir[z]; jobs.nw[jobs.n] = fl.stage[2 + z]; jobs.xh[jobs.n] = b.hist_tail[z];
        jobs.corr[jobs.n] = fl.corr[4 + z]; jobs.C[jobs.n] = M; jid[jobs.n++] = 4 + z;
    }
    if (jobs.n == 0) return APV_OK;
    LCHK(h, apv_launch_fir_tail(b.f64, jobs, P, st));
    // only now may the old banks go
    for (int z = 0; z < 2; ++z)
        if (h_new[z]) LCHK(h, hipMemcpyAsync(b.rir[z], fl.stage[z], esz * (size_t)P * C, hipMemcpyDeviceToDevice, st));
    for (int z = 0; z < 2; ++z)
        if (h_new[2 + z]) LCHK(h, hipMemcpyAsync(b.trir[z], fl.stage[2 + z], esz * (size_t)P * M, hipMemcpyDeviceToDevice, st));
    for (int i = 0; i < jobs.n; ++i) fl.live[jid[i]] = true;
    if (P > 1) fl.hops_left = std::max(fl.hops_left, (P - 1 + H - 1) / H);
    return APV_OK;
}

int apv_live_apply(apv_handle* h, FirLive& fl, int P, int C, int M, int f64, void* const dst[6], int n_add, int shift, long row_len,
                   int d0, int dmod, hipStream_t st) {
    if (fl.hops_left <= 0) return APV_OK;
    FirLiveJobs jobs{};
    for (int j = 0; j < 6; ++j) {
        if (!fl.live[j]) continue;
        jobs.corr[jobs.n] = fl.corr[j]; jobs.dst[jobs.n] = dst[j]; jobs.C[jobs.n++] = j < 4 ? C : M;
    }
    LCHK(h, apv_launch_tail_apply(f64, jobs, P - 1, n_add, shift, row_len, d0, dmod, st));
    return APV_OK;
}

void apv_live_advance(FirLive& fl, int hops) {
    if (fl.hops_left <= 0) return;
    fl.hops_left = std::max(0, fl.hops_left - hops);
    if (fl.hops_left == 0)
        for (bool& l : fl.live) l = false;     // every tail has been shifted out: the buffers hold zeros
}

int apv_live_state(apv_handle* h, FirLive& fl, int j, int P, int H, int C, int M, size_t esz, void* h_buf, size_t bytes, bool get,
                   hipStream_t st) {
    const int rows = j < 4 ? C : M, Q = std::max(P - 1, 1);
    const size_t need = esz * (size_t)rows * Q;
    if (bytes != need) return apv_fail(h, APV_ERR_STATE, "state size mismatch");
    if (get) {
        if (!fl.corr[0]) {
            std::memset(h_buf, 0, bytes);                   // never updated: no tail
            return APV_OK;
        }
        LCHK(h, hipMemcpyAsync(h_buf, fl.corr[j], bytes, hipMemcpyDeviceToHost, st));
        LCHK(h, hipStreamSynchronize(st));
        return APV_OK;
    }
    // the hops this tail still reaches: up to its last nonzero sample
    int last = -1;
    for (int r = 0; r < rows; ++r)
        for (int n = Q - 1; n > last; --n) {
            const char* e = (const char*)h_buf + ((size_t)r * Q + n) * esz;
            const bool nz = esz == 8 ? *(const double*)e != 0.0 : *(const float*)e != 0.0f;
            if (nz) { last = n; break; }
        }
    if (last < 0 && !fl.corr[0]) return APV_OK;            // a zero tail into a stream that has none: nothing to keep
    int rc = apv_live_alloc(h, fl, P, C, M, esz, st);
    if (rc != APV_OK) return rc;
    LCHK(h, hipMemcpyAsync(fl.corr[j], h_buf, bytes, hipMemcpyHostToDevice, st));
    LCHK(h, hipStreamSynchronize(st));
    if (last >= 0) {
        fl.live[j] = true;
        fl.hops_left = std::max(fl.hops_left, (last + H) / H);
    }
    return APV_OK;
}
