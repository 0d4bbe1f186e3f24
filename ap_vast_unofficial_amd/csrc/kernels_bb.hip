// Kernels of the broadband (time-domain) stream, float64, behind the apv_launch_* prototypes of apv_internal.h: input histories
// and rings, the Hankel statistics R and r (apvast.py:329-364), the relative loading, the output products and the evaluation's
// pressure prediction.  stream_bb.hip says when each runs; capi.hip uses the statistics for the static solver.
#include "apv_internal.h"

namespace {

using d4 = __attribute__((ext_vector_type(4))) double;

// both input signals' histories in one launch (blockIdx.y = signal)
__global__ void __launch_bounds__(256) hist2_f64_kernel(int P, int H, int pad, const double* __restrict__ old0,
                                                        const double* __restrict__ old1, const double* __restrict__ x,
                                                        double* __restrict__ new0, double* __restrict__ new1) {
    const int g = blockIdx.y;
    const double* old_hist = g ? old1 : old0;
    double* new_hist = g ? new1 : new0;
    x += (size_t)g * H;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int keep = P - 1;
    if (i < keep) new_hist[i] = old_hist[i + H];
    else if (i < keep + H) new_hist[i] = x[i - keep];
    else if (i < keep + H + pad) new_hist[i] = 0.0;
}

// ring[c][(len - H + n + off) % len] = src[c][n], n < H   (src row stride src_ld)
__global__ void __launch_bounds__(256) ring_append_f64_kernel(int len, int H, int off, const double* __restrict__ src,
                                                              long src_ld, double* __restrict__ ring) {
    const int c = blockIdx.y;
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < H) ring[(size_t)c * len + (len - H + n + off) % len] = src[(size_t)c * src_ld + n];
}

// ---- statistics -----------------------------------------------------------------------------------
// logical sample t of the "toeplitz" sequence g = buf with sample J removed (apvast.py:336-338)
// (skip = 0: plain Hankel data matrix, used by the static solver)
__device__ __forceinline__ double stat_at(const double* __restrict__ ring, int S, int off, int J, int t, int skip = 1) {
    const int u = (t < J || !skip) ? t : t + 1;
    int ph = u + off;
    if (ph >= S) ph -= S;
    return ring[ph];
}


// R[rho][sigma] = sum_m sum_ncol Y_m[rho][ncol] Y_m[sigma][ncol], Y_m[(s, i)][ncol] = g_{s,m}[J-1-i+ncol].
//
// A workgroup of four waves owns a 32 x 32 tile of R (one 16 x 16 v_mfma_f64_16x16x4_f64 accumulator per wave).
// A row (s, i) of Y is a window of the sequence g_{s,m}, so a tile side only ever needs, per microphone and per
// chunk of TC columns, one window of TC + 31 samples for each loudspeaker its 32 rows touch: those windows are
// unwrapped from the rings into LDS once (double-buffered: the next set is fetched into registers while the MFMAs
// of the current one run) and every operand is then an LDS read at (window base + column).
constexpr int SY_PER = 10;                      // window doubles staged per thread and step
constexpr int SY_BUF = 256 * SY_PER;            // doubles per LDS buffer (both sides, all segments)

__global__ void __launch_bounds__(256) syrk_hankel_kernel(int n, int J, int L, int M, int S, int off, int skip, int ncols,
                                                          int TC, int nseg, SyrkJobs jobs) {
    extern __shared__ double sy_lds[];           // [2][SY_BUF]
    const double* __restrict__ stats = jobs.stats[blockIdx.z];
    double* __restrict__ R = jobs.R[blockIdx.z];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int W = TC + 32;
    const int nchunks = (ncols + TC - 1) / TC, iters = M * nchunks;
    const int tmax = skip ? S - 2 : S - 1;
    const int slo[2] = {r0 / J, c0 / J};
    const int t0[2] = {r0, c0};
    // this lane's rows on the two sides of its wave tile
    const int ra = r0 + (wave >> 1) * 16 + (lane & 15), cb = c0 + (wave & 1) * 16 + (lane & 15);
    int offA = -1, offB = -1;
    if (ra < n) {
        const int sa = ra / J, ia = ra - sa * J;
        const int ihi = min(r0 + 31, (sa + 1) * J - 1) - sa * J;
        offA = (sa - slo[0]) * W + (ihi - ia) + kq;
    }
    if (cb < n) {
        const int sb = cb / J, ib = cb - sb * J;
        const int ihi = min(c0 + 31, (sb + 1) * J - 1) - sb * J;
        offB = (nseg + sb - slo[1]) * W + (ihi - ib) + kq;
    }
    // staging: element e of the buffer = (side, segment, w)
    const int total = 2 * nseg * W;
    double stage[SY_PER];
    auto fetch = [&](int it) {
        const int m = it / nchunks, nc0 = (it - m * nchunks) * TC;
#pragma unroll
        for (int q = 0; q < SY_PER; ++q) {
            const int e = tid + q * 256;
            double v = 0.0;
            if (e < total) {
                const int sg = e / W, w = e - sg * W;
                const int side = sg >= nseg, sp = slo[side] + (side ? sg - nseg : sg);
                if (sp < L) {
                    const int ihi = min(t0[side] + 31, (sp + 1) * J - 1) - sp * J;
                    const int t = nc0 + J - 1 - ihi + w;
                    if (t <= tmax && ihi >= 0) v = stat_at(stats + (size_t)(m * L + sp) * S, S, off, J, t, skip);
                }
            }
            stage[q] = v;
        }
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int q = 0; q < SY_PER; ++q) {
            const int e = tid + q * 256;
            if (e < total) sy_lds[buf * SY_BUF + e] = stage[q];
        }
    };
    d4 acc = {0, 0, 0, 0};
    fetch(0);
    commit(0);
    __syncthreads();
    for (int it = 0; it < iters; ++it) {
        const int buf = it & 1;
        if (it + 1 < iters) fetch(it + 1);
        const int nc0 = (it % nchunks) * TC;
        const int steps = (min(TC, ncols - nc0) + 3) >> 2;
        const double* la = sy_lds + buf * SY_BUF + (offA >= 0 ? offA : 0);
        const double* lb = sy_lds + buf * SY_BUF + (offB >= 0 ? offB : 0);
        const bool tail = nc0 + 4 * steps > ncols;          // the last step of the last chunk may run past the columns
        const int full_steps = tail ? steps - 1 : steps;
        int k = 0;
        for (; k + 4 <= full_steps; k += 4) {
            const double a0 = la[4 * k], a1 = la[4 * k + 4], a2 = la[4 * k + 8], a3 = la[4 * k + 12];
            const double b0 = lb[4 * k], b1 = lb[4 * k + 4], b2 = lb[4 * k + 8], b3 = lb[4 * k + 12];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(offA >= 0 ? a0 : 0.0, offB >= 0 ? b0 : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(offA >= 0 ? a1 : 0.0, offB >= 0 ? b1 : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(offA >= 0 ? a2 : 0.0, offB >= 0 ? b2 : 0.0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(offA >= 0 ? a3 : 0.0, offB >= 0 ? b3 : 0.0, acc, 0, 0, 0);
        }
        for (; k < steps; ++k) {
            const bool ok = nc0 + 4 * k + kq < ncols;
            const double a = (ok && offA >= 0) ? la[4 * k] : 0.0;
            const double b = (ok && offB >= 0) ? lb[4 * k] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        if (it + 1 < iters) commit(buf ^ 1);
        __syncthreads();
    }
    // f64 accumulator: row = (lane>>4) + 4 t, col = lane & 15
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int row = r0 + (wave >> 1) * 16 + kq + 4 * t, col = c0 + (wave & 1) * 16 + (lane & 15);
        if (row < n && col < n) R[(size_t)row * n + col] = acc[t];
    }
}

// ---- the same statistics from the displacement structure of the data matrix (round 4) ---------------------------------------
// Row (s, i) of Y_m is the window of g_{s,m} that starts at u = J - 1 - i, so R[(s, i), (s', i')] = E(u, u') =
// sum_m sum_{n < ncols} g_{s,m}[u + n] g_{s',m}[u' + n] depends on the lag d = u' - u and, weakly, on where the window sits:
// E(u + 1, u' + 1) = E(u, u') - sum_m g_s[u] g_s'[u'] + sum_m g_s[u + ncols] g_s'[u' + ncols].  One full sum per lag (2 J - 1 of
// them per pair of loudspeakers) and a walk down each diagonal replace J^2 full sums: (2 J - 1)(ncols + 2 J) instead of J^2 ncols
// multiply-adds per pair and microphone -- 16 x fewer at J = 32, 41 x at J = 100 (apvast.py:334-347 forms Y and Y Y^T outright;
// numpy's own summation order differs from any of these by the same few ulp).  A workgroup owns a pair (s <= s') of one
// matrix: the unwrapped sequences of all microphones of both loudspeakers sit in LDS (2 M (S + 8) doubles: 128 KB at the
// reference's parameters); the full sums take four consecutive lags per thread (one new LDS read per lag block and sample)
// and split the column range over the thread groups; the walks take one lag per thread.  R's mirror image is written too.
constexpr int HC_TPB = 1024, HC_MAXPARTS = 10, HC_MAXSEG = 16;
// doubles of the work array behind the sequences: the full sums' partials [parts][lag blocks][4], later the walks' segment sums
__host__ __device__ inline int hc_red_len(int J) {
    const int nbk = (J + 3) / 4 + (J - 1 + 3) / 4, nqmax = 2 * J - 1;
    int nseg = HC_TPB / nqmax;
    nseg = nseg < 1 ? 1 : (nseg > HC_MAXSEG ? HC_MAXSEG : nseg);
    const int a = HC_MAXPARTS * nbk * 4, b = nqmax * nseg;
    return a > b ? a : b;
}
__global__ void __launch_bounds__(HC_TPB) hankel_corr_kernel(int n, int J, int L, int M, int S, int off, int skip, int ncols, int Sg,
                                                             SyrkJobs jobs) {
    extern __shared__ double hc_lds[];           // g[2][M][Sg], then red[parts][NBK][4] (later: seg[nq][nseg]), then e0[2 J]
    const double* __restrict__ stats = jobs.stats[blockIdx.z];
    double* __restrict__ R = jobs.R[blockIdx.z];
    const int tid = threadIdx.x;
    int sa = 0, sb = blockIdx.x;                  // pair index -> s <= s'
    while (sb >= L - sa) { sb -= L - sa; ++sa; }
    sb += sa;
    const bool same = sa == sb;
    const int tmax = skip ? S - 2 : S - 1;
    double* const gA = hc_lds;
    double* const gB = hc_lds + (size_t)M * Sg;
    for (int e = tid; e < 2 * M * Sg; e += HC_TPB) {
        const int side = e / (M * Sg), r = e - side * M * Sg, m = r / Sg, t = r - m * Sg;
        const int sp = side ? sb : sa;
        hc_lds[e] = t <= tmax ? stat_at(stats + (size_t)(m * L + sp) * S, S, off, J, t, skip) : 0.0;
    }
    __syncthreads();
    // lag jobs: q < J: d = q >= 0 (A = g_s, B = g_s', u = 0, u' = d); q >= J: d = -(q - J + 1) (A = g_s', B = g_s, u' = 0, u = -d)
    const int nq = same ? J : 2 * J - 1;
    const int nb_pos = (J + 3) / 4, nb_neg = same ? 0 : (J - 1 + 3) / 4, NBK = nb_pos + nb_neg;
    int parts = HC_TPB / NBK;
    parts = parts < 1 ? 1 : (parts > HC_MAXPARTS ? HC_MAXPARTS : parts);
    double* const red = hc_lds + (size_t)2 * M * Sg;                 // [parts][NBK][4]; the walks reuse it as seg[nq][nseg]
    const int red_len = hc_red_len(J);
    double* const e0 = red + red_len;                                 // [2 J]
    for (int item = tid; item < NBK * parts; item += HC_TPB) {
        // neighbouring lanes take neighbouring column ranges of the same lag block, an ODD number of samples apart: their LDS reads
        // fall into different banks (lanes on neighbouring lag blocks read 32 bytes apart: a four-way conflict on every access)
        const int part = item % parts, blk = item / parts;
        const bool neg = blk >= nb_pos;
        const int dd0 = neg ? 1 + 4 * (blk - nb_pos) : 4 * blk;
        const double* const A = neg ? gB : gA;
        const double* const B = neg ? gA : gB;
        const int per = ((ncols + parts - 1) / parts) | 1, n0 = min(ncols, part * per), n1 = min(ncols, n0 + per);
        double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int m = 0; m < M; ++m) {
            const double* const Am = A + (size_t)m * Sg;
            const double* const Bm = B + (size_t)m * Sg + dd0;
            if (n0 < n1) {
                double b0 = Bm[n0], b1 = Bm[n0 + 1], b2 = Bm[n0 + 2];
#pragma unroll 4
                for (int nn = n0; nn < n1; ++nn) {
                    const double b3 = Bm[nn + 3], a = Am[nn];
                    a0 = __builtin_fma(a, b0, a0);
                    a1 = __builtin_fma(a, b1, a1);
                    a2 = __builtin_fma(a, b2, a2);
                    a3 = __builtin_fma(a, b3, a3);
                    b0 = b1; b1 = b2; b2 = b3;
                }
            }
        }
        double* o = red + ((size_t)part * NBK + blk) * 4;
        o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
    }
    __syncthreads();
    for (int q = tid; q < nq; q += HC_TPB) {
        const bool neg = q >= J;
        const int dd = neg ? q - J + 1 : q;
        const int blk = neg ? nb_pos + (dd - 1) / 4 : dd / 4, sub = neg ? (dd - 1) % 4 : dd % 4;
        double v = 0.0;
        for (int part = 0; part < parts; ++part) v += red[((size_t)part * NBK + blk) * 4 + sub];
        e0[q] = v;
    }
    __syncthreads();
    // The walks, E(u + 1, u' + 1) = E(u, u') + delta(u), cut into nseg segments per diagonal so that every thread has one: first
    // every segment's sum of deltas, then each segment starts from e0 plus the sums of the segments before it (fixed order) and
    // walks, forming its deltas a second time (twice the multiply-adds, nseg times the threads).
    int nseg = HC_TPB / nq;
    nseg = nseg < 1 ? 1 : (nseg > HC_MAXSEG ? HC_MAXSEG : nseg);
    const int seglen = ((J + nseg - 1) / nseg) | 1;            // odd: the segments of a diagonal start in different LDS banks
    auto delta = [&](const double* A, const double* B, int dd, int u) {
        double dl = 0.0;
        for (int m = 0; m < M; ++m) {
            const double* const Am = A + (size_t)m * Sg;
            const double* const Bm = B + (size_t)m * Sg;
            dl = __builtin_fma(Am[u + ncols], Bm[u + dd + ncols], dl);
            dl = __builtin_fma(-Am[u], Bm[u + dd], dl);
        }
        return dl;
    };
    double* const seg = red;
    for (int item = tid; item < nq * nseg; item += HC_TPB) {
        const int q = item / nseg, g = item - q * nseg;
        const bool neg = q >= J;
        const int dd = neg ? q - J + 1 : q, len = J - dd;
        const double* const A = neg ? gB : gA;
        const double* const B = neg ? gA : gB;
        double sum = 0.0;
        for (int u = g * seglen; u < (g + 1) * seglen && u + 1 < len; ++u) sum += delta(A, B, dd, u);
        seg[(size_t)q * nseg + g] = sum;
    }
    __syncthreads();
    for (int item = tid; item < nq * nseg; item += HC_TPB) {
        const int q = item / nseg, g = item - q * nseg;
        const bool neg = q >= J;
        const int dd = neg ? q - J + 1 : q, len = J - dd;
        const double* const A = neg ? gB : gA;
        const double* const B = neg ? gA : gB;
        double E = e0[q];
        for (int gp = 0; gp < g; ++gp) E += seg[(size_t)q * nseg + gp];
        for (int u = g * seglen; u < (g + 1) * seglen && u < len; ++u) {
            // A's window starts at u, B's at u + dd: rows i = J - 1 - start
            const int iA = J - 1 - u, iB = J - 1 - (u + dd);
            const int row = (neg ? sb : sa) * J + iA, col = (neg ? sa : sb) * J + iB;
            R[(size_t)row * n + col] = E;
            R[(size_t)col * n + row] = E;
            if (u + 1 < len) E += delta(A, B, dd, u);
        }
    }
}

// window length and segment count that fit the staging buffer for this (J, S)
static void syrk_plan(int J, int ncols, int* TC, int* nseg) {
    *nseg = 31 / J + 2;                                   // loudspeakers a run of 32 rows can touch
    int W = SY_BUF / (2 * *nseg);
    int tc = ((W - 32) / 4) * 4;
    const int ncols4 = (ncols + 3) / 4 * 4;
    if (tc > ncols4) tc = ncols4;
    if (tc < 4) tc = 4;
    *TC = tc;
}

// r[rho] = sum_m sum_ncol Y_m[rho][ncol] d_m[toff + ncol]      (apvast.py:340, 356: toff = J; apVast.m:425: J - 1)
__global__ void __launch_bounds__(256) xcorr_hankel_kernel(int n, int J, int L, int M, int S, int off, int skip, int ncols,
                                                           int toff, const double* __restrict__ stats,
                                                           const double* __restrict__ tstats, double* __restrict__ r) {
    const int rho = blockIdx.x;
    const int s = rho / J, i = rho % J;
    double acc = 0.0;
    for (int idx = threadIdx.x; idx < M * ncols; idx += 256) {
        const int m = idx / ncols, nc = idx - m * ncols;
        const double y = stat_at(stats + (size_t)(m * L + s) * S, S, off, J, J - 1 - i + nc, skip);
        int ph = toff + nc + off;
        if (ph >= S) ph -= S;
        acc += y * tstats[(size_t)m * S + ph];
    }
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) r[rho] = red[0];
}

// R[i][i] += coef * nrm[q]
__global__ void __launch_bounds__(256) add_rel_diag_kernel(int n, double* __restrict__ R, double coef, const double* __restrict__ nrm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) R[(size_t)i * n + i] += coef * nrm[0];
}

// out[ch][k] = in[k] * filt[ch][k]   (complex, channel-major) for up to four channel groups with inputs of their own
__global__ void __launch_bounds__(256) apply_f64_jobs_kernel(int K, ApplyJobsD j) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    int ch = blockIdx.y, q = 0;
    while (q + 1 < j.n && ch >= j.first[q + 1]) ++q;
    ch -= j.first[q];
    if (k >= K) return;
    const double2 x = j.in[q][k], f = j.filt[q][(size_t)ch * K + k];
    j.out[q][(size_t)ch * K + k] = make_double2(x.x * f.x - x.y * f.y, x.x * f.y + x.y * f.x);
}

// p[t][m] = sum_s sum_q rir[q][s][m] x[t-q][s]          (Matlab/ControlMethods/predictPressure.m:12-16)
__global__ void __launch_bounds__(256) predict_pressure_kernel(int T, int L, int M, int P, const double* __restrict__ x,
                                                               const double* __restrict__ rir, double* __restrict__ out) {
    const int m = threadIdx.x % M, tl = threadIdx.x / M;
    const int tpb = 256 / M;
    const int t = blockIdx.x * tpb + tl;
    if (tl >= tpb || t >= T) return;
    double acc = 0.0;
    const int qmax = (t + 1 < P) ? t + 1 : P;
    for (int q = 0; q < qmax; ++q) {
        const double* xr = x + (size_t)(t - q) * L;
        const double* rr = rir + (size_t)q * L * M + m;
        for (int s = 0; s < L; ++s) acc = __builtin_fma(rr[(size_t)s * M], xr[s], acc);
    }
    out[(size_t)t * M + m] = acc;
}

__global__ void __launch_bounds__(256) scale_kernel(size_t count, double* __restrict__ v, double f) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) v[i] *= f;
}

}  // namespace

hipError_t apv_launch_hist2_f64(int P, int H, int pad, const double* old0, const double* old1, const double* x, double* new0,
                                double* new1, hipStream_t s) {
    hipLaunchKernelGGL(hist2_f64_kernel, dim3((P - 1 + H + pad + 255) / 256, 2), dim3(256), 0, s, P, H, pad, old0, old1, x, new0, new1);
    return hipGetLastError();
}

hipError_t apv_launch_ring_append_f64(int len, int H, int off, const double* src, long src_ld, double* ring, int n_ch, hipStream_t s) {
    hipLaunchKernelGGL(ring_append_f64_kernel, dim3((H + 255) / 256, n_ch), dim3(256), 0, s, len, H, off, src, src_ld, ring);
    return hipGetLastError();
}

hipError_t apv_launch_syrk_hankel(hipStream_t st, int n, int J, int L, int M, int S, int off, int skip, int ncols, int njobs,
                                  const SyrkJobs& jobs, int form, int* form_taken) {
    // the displacement form where its LDS fits (both loudspeakers' sequences of all microphones) and a thread has a lag block,
    // else the dense products on the matrix cores; `form` forces one of the two (apv_hankel_statistics)
    const int Sg = S + 8;
    const size_t lds = sizeof(double) * ((size_t)2 * M * Sg + (size_t)hc_red_len(J) + 2 * (size_t)J);
    const bool fits = 2 * J - 1 <= HC_TPB && lds <= 158 * 1024 && ncols + J + 2 <= Sg;
    if (form == APV_HANKEL_DISPLACEMENT && !fits) return hipErrorInvalidValue;
    const bool displacement = fits && form != APV_HANKEL_DENSE;
    if (form_taken) *form_taken = displacement ? APV_HANKEL_DISPLACEMENT : APV_HANKEL_DENSE;
    if (displacement) {
        static std::atomic<unsigned long long> attr_set{0};
        const hipError_t e = apv_set_max_dynamic_lds(reinterpret_cast<const void*>(&hankel_corr_kernel), 158 * 1024, attr_set);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hankel_corr_kernel, dim3(L * (L + 1) / 2, 1, njobs), dim3(HC_TPB), lds, st, n, J, L, M, S, off, skip, ncols, Sg, jobs);
        return hipGetLastError();
    }
    int TC, nseg;
    syrk_plan(J, ncols, &TC, &nseg);
    hipLaunchKernelGGL(syrk_hankel_kernel, dim3((n + 31) / 32, (n + 31) / 32, njobs), dim3(256), sizeof(double) * 2 * SY_BUF, st, n, J,
                       L, M, S, off, skip, ncols, TC, nseg, jobs);
    return hipGetLastError();
}

hipError_t apv_launch_xcorr_hankel(int n, int J, int L, int M, int S, int off, int skip, int ncols, int toff, const double* stats,
                                   const double* tstats, double* r, hipStream_t s) {
    hipLaunchKernelGGL(xcorr_hankel_kernel, dim3(n), dim3(256), 0, s, n, J, L, M, S, off, skip, ncols, toff, stats, tstats, r);
    return hipGetLastError();
}

hipError_t apv_launch_add_rel_diag(int n, double* R, double coef, const double* nrm, hipStream_t s) {
    hipLaunchKernelGGL(add_rel_diag_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, R, coef, nrm);
    return hipGetLastError();
}

hipError_t apv_launch_apply_jobs_f64(int K, const ApplyJobsD& j, hipStream_t s) {
    hipLaunchKernelGGL(apply_f64_jobs_kernel, dim3((K + 255) / 256, j.first[j.n]), dim3(256), 0, s, K, j);
    return hipGetLastError();
}

hipError_t apv_launch_predict_pressure(int T, int L, int M, int P, const double* x, const double* rir, double* out, hipStream_t s) {
    const int tpb = 256 / M;
    hipLaunchKernelGGL(predict_pressure_kernel, dim3((T + tpb - 1) / tpb), dim3(256), 0, s, T, L, M, P, x, rir, out);
    return hipGetLastError();
}

hipError_t apv_launch_scale_f64(size_t count, double* v, double f, hipStream_t s) {
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, count, v, f);
    return hipGetLastError();
}
