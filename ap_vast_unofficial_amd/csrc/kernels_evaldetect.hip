// Perceptual detectability of the evaluated pressures (apv_stream_set_evaluation_detectability): the second half of the masking
// model, evaluateDetectability (Matlab/ControlMethods/perceptualModel.m:192-206), behind the per-bin spectra of
// kernels_evalspec.hip and on their bin-major scratch spec [K][Z (2 E + 1) Mv] complex128 (per program z: B[z, e] bright, Dk[z, e]
// dark, T[z] target).  With f = 2 / N^2, G2 [K][C] the squared channel responses and the squared weighting curve of a masker S
//
//   w2_S[k] = Cs Leff sum_c G2[k, c] / (f sum_j G2[j, c] |S[j]|^2 + Ca)                  (perceptualModel.m:118-139; j from 0)
//   error[z, e, m] = sum_{k >= 1} w2_{T[z, m]}[k] f |T[z, m, k] - B[z, e, m, k]|^2
//   leak [z, e, m] = sum_{k >= 1} w2_{T[1 - z, m]}[k] f |Dk[z, e, m, k]|^2               (Z = 1: the masker is silence)
//
// Through the curves, not through the channel powers of every disturbance.  Three launches, everything float64:
//
// 1. eval_detect_curve_kernel.  One workgroup of 1024 threads per target column (z, m) -- Z Mv workgroups are fewer than the CUs, so
// a curve's parallelism has to come from inside its workgroup: f |T[k]|^2 of the K bins into LDS; wave w of the 16 forms the masker
// power of the channels w, w + 16, ... (lanes along the bins of the channel-major table G2T [C][K], four independent partial sums
// per lane so that four loads are in flight, combined pairwise and summed over the lanes by a shuffle tree) and leaves
// 1 / (masker + Ca) in LDS; then one thread per bin sums G2T[c][k] inv[c] over the channels in ascending order and writes the
// UN-normalised w2[k] to curves [K][Z Mv], microphones fastest.  perceptual_weights_kernel
// (kernels_stream.hip) is the model; the table (360 KB at K = 1025, C = 44) is streamed from L2, both passes with neighbouring
// lanes on neighbouring bins.  Thread 0 of workgroup 0 advances the hop counter ctl[2] of the per-call record.  Launched once per
// stream without spectra, it gives the curve of a silent masker.
//
// 2. eval_detect_reduce_kernel.  A workgroup owns 16 microphones of one (program, rank) and one chunk of the bins 1 .. K - 1: thread
// (slice = tid >> 4, lane microphone = tid & 15) walks the chunk's bins slice, slice + 16, ... with both disturbances (the target's
// bin is read once), neighbouring lanes on neighbouring microphones of the scratch and of the curves; the 16 slices are summed by
// an LDS tree and the two partial sums go to part [chunks][Z][2 E][Mv].  The chunks -- a function of the sizes alone -- fill the
// device where one thread per row would leave it empty (cfg3, one rank: 128 rows).
//
// 3. eval_detect_update_kernel.  One thread per (program, error | leak, rank, microphone) adds the chunks in ascending order, writes
// the hop's slot and updates sum (total = total + hop), max and the count of D > 1 in totals [Z][6 E][Mv].
//
// No atomics, every combination order fixed: the bits depend on the sizes and the data alone.  Bounds: every access is predicated;
// K, Mv, E, C need not be multiples of anything.  Nothing is read past [K][Z (2 E + 1) Mv] spectra, [C][K] table entries and
// [K][Z Mv] curves, nothing written past the curves, [chunks][Z][2 E][Mv] partial sums, the record's slots and the totals.
//
// The hop-batched forms (apv_launch_eval_detect_hops; the broadband stream, whose scratch holds the spectra of c consecutive hops
// [c][K][Z (2 E + 1) Mv]) are the same three bodies with the hop as one more grid coordinate: c Z Mv curve workgroups into curves
// [c][K][Z Mv], the reduction's workgroups c times over into part [c][chunks][Z][2 E][Mv] -- chunks and the slice walk are those of
// one hop, so a hop's partial sums do not know the launch they are in --, and ONE update launch whose threads walk the c hops in
// order: chunks ascending, the record's slot slot0 + i (a launch argument), then sum, max and count carried in registers.  The bits
// of a hop and of the totals therefore depend on the sizes, the data and the hop order alone, and at c = 1 they are those of the
// per-hop launches: both forms compile the same device functions.
#include "apv_internal.h"

#include <algorithm>

namespace {

constexpr int ED_T = 16;                       // microphones of a workgroup of the reduction = bin slices of it
constexpr int ED_FILL = 256;                   // workgroups the reduction aims for: one per CU
constexpr int ED_CT = 1024;                    // threads of a workgroup of the curve kernel

// the curve of target column `col` = (z, m) of one hop's spectra (null: silence) into curves[k c_k + col]
__device__ __forceinline__ void curve_column(const double2* __restrict__ spec, int Z, int E, int K, int Mv, int C,
                                             const double* __restrict__ G2T, double Cs, double Ca, double Leff, double f,
                                             double* __restrict__ curves, long c_k, int col) {
    extern __shared__ double ed_sm[];
    double* P2 = ed_sm;                        // [K]
    double* inv = ed_sm + K;                   // [C]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int z = col / Mv, m = col - z * Mv;
    if (spec) {
        const size_t row = (size_t)Z * (2 * E + 1) * Mv;
        const double2* __restrict__ t = spec + ((size_t)z * (2 * E + 1) + 2 * E) * Mv + m;
        for (int k = tid; k < K; k += ED_CT) {
            const double2 v = t[(size_t)k * row];
            P2[k] = f * (v.x * v.x + v.y * v.y);
        }
    } else {
        for (int k = tid; k < K; k += ED_CT) P2[k] = 0.0;
    }
    __syncthreads();
    for (int c = wave; c < C; c += ED_CT / 64) {
        const double* __restrict__ g = G2T + (size_t)c * K;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        int k = lane;
        for (; k + 192 < K; k += 256) {
            a0 += g[k] * P2[k];
            a1 += g[k + 64] * P2[k + 64];
            a2 += g[k + 128] * P2[k + 128];
            a3 += g[k + 192] * P2[k + 192];
        }
        for (; k < K; k += 64) a0 += g[k] * P2[k];
        double a = (a0 + a1) + (a2 + a3);
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
        if (lane == 0) inv[c] = 1.0 / (a + Ca);
    }
    __syncthreads();
    const double scale = Cs * Leff;
    for (int k = tid; k < K; k += ED_CT) {
        double a = 0.0;
#pragma unroll 4
        for (int c = 0; c < C; ++c) a += G2T[(size_t)c * K + k] * inv[c];
        curves[(size_t)k * c_k + col] = a * scale;
    }
}

__global__ void __launch_bounds__(ED_CT) eval_detect_curve_kernel(const double2* __restrict__ spec, int Z, int E, int K, int Mv, int C,
                                                                const double* __restrict__ G2T, double Cs, double Ca, double Leff,
                                                                double f, double* __restrict__ curves, long c_k,
                                                                unsigned long long* __restrict__ ctl) {
    if (ctl && blockIdx.x == 0 && threadIdx.x == 0) ctl[2] = ctl[2] + 1;     // no other thread of this launch reads it
    curve_column(spec, Z, E, K, Mv, C, G2T, Cs, Ca, Leff, f, curves, c_k, (int)blockIdx.x);
}

// the hop-batched form: workgroup (column, hop) of spec [c][K][Z (2 E + 1) Mv] into curves [c][K][Z Mv]
__global__ void __launch_bounds__(ED_CT) eval_detect_curve_hops_kernel(const double2* __restrict__ spec, int Z, int E, int K, int Mv, int C,
                                                                     const double* __restrict__ G2T, double Cs, double Ca, double Leff,
                                                                     double f, double* __restrict__ curves) {
    const size_t c_k = (size_t)Z * Mv, hop = blockIdx.y;
    curve_column(spec + hop * K * ((size_t)Z * (2 * E + 1) * Mv), Z, E, K, Mv, C, G2T, Cs, Ca, Leff, f, curves + hop * K * c_k,
                 (long)c_k, (int)blockIdx.x);
}

// the partial sums of microphone group mg of (program, rank) zy over the bins of chunk ch of one hop: spec, curves and part are
// the hop's own
__device__ __forceinline__ void reduce_chunk(const double2* __restrict__ spec, const double* __restrict__ curves,
                                             const double* __restrict__ quiet, double* __restrict__ part, int Z, int E, int K, int Mv,
                                             int kc, double f, int mg, int zy, int ch) {
    __shared__ double red[2][ED_T][ED_T + 1];
    const int tid = threadIdx.x, ml = tid & 15, sl = tid >> 4;
    const int z = zy / E, e = zy - z * E, m = mg * ED_T + ml;
    const int k0 = 1 + ch * kc, k1 = min(K, k0 + kc);
    double err = 0.0, leak = 0.0;
    if (m < Mv) {
        const size_t row = (size_t)Z * (2 * E + 1) * Mv, cw = (size_t)Z * Mv;
        const double2* __restrict__ sz = spec + (size_t)z * (2 * E + 1) * Mv + m;
        const double* __restrict__ wt = curves + (size_t)z * Mv + m;             // the curve of this program's target here
        // the curve of the other program's target at the same microphone; with one program, that of silence
        const double* __restrict__ wl = Z == 2 ? curves + (size_t)(1 - z) * Mv + m : quiet;
        const size_t wl_k = Z == 2 ? cw : 1;
        for (int k = k0 + sl; k < k1; k += ED_T) {
            const double2* __restrict__ sk = sz + (size_t)k * row;
            const double2 t = sk[(size_t)2 * E * Mv], br = sk[(size_t)e * Mv], dk = sk[(size_t)(E + e) * Mv];
            const double dx = t.x - br.x, dy = t.y - br.y;
            err += wt[(size_t)k * cw] * (f * (dx * dx + dy * dy));
            leak += wl[(size_t)k * wl_k] * (f * (dk.x * dk.x + dk.y * dk.y));
        }
    }
    red[0][sl][ml] = err;
    red[1][sl][ml] = leak;
    __syncthreads();
    for (int w = ED_T / 2; w > 0; w >>= 1) {
        if (sl < w) {
            red[0][sl][ml] += red[0][sl + w][ml];
            red[1][sl][ml] += red[1][sl + w][ml];
        }
        __syncthreads();
    }
    if (sl < 2 && m < Mv) {
        const size_t items = (size_t)Z * 2 * E * Mv;
        part[(size_t)ch * items + ((size_t)z * 2 * E + (size_t)sl * E + e) * Mv + m] = red[sl][0][ml];
    }
}

__global__ void __launch_bounds__(256) eval_detect_reduce_kernel(const double2* __restrict__ spec, const double* __restrict__ curves,
                                                                 const double* __restrict__ quiet, double* __restrict__ part, int Z,
                                                                 int E, int K, int Mv, int kc, double f) {
    reduce_chunk(spec, curves, quiet, part, Z, E, K, Mv, kc, f, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z);
}

// the hop-batched form: blockIdx.x = hop x microphone groups + group, so that the hops are bounded by 2^31 and not by 65535;
// spec [c][K][Z (2 E + 1) Mv], curves [c][K][Z Mv], part [c][chunks][Z][2 E][Mv]
__global__ void __launch_bounds__(256) eval_detect_reduce_hops_kernel(const double2* __restrict__ spec, const double* __restrict__ curves,
                                                                      const double* __restrict__ quiet, double* __restrict__ part, int Z,
                                                                      int E, int K, int Mv, int kc, double f, int groups) {
    const size_t hop = blockIdx.x / (unsigned)groups;
    const int mg = (int)(blockIdx.x - hop * groups);
    reduce_chunk(spec + hop * K * ((size_t)Z * (2 * E + 1) * Mv), curves + hop * K * ((size_t)Z * Mv), quiet,
                 part + hop * gridDim.z * ((size_t)Z * 2 * E * Mv), Z, E, K, Mv, kc, f, mg, (int)blockIdx.y, (int)blockIdx.z);
}

// sum, max and count of D > 1 of element `it` of a hop, one hop later
__device__ __forceinline__ void fold_hop(double d, double& sum, double& mx, double& cnt) {
    sum = sum + d;
    mx = d > mx ? d : mx;
    cnt = cnt + (d > 1.0 ? 1.0 : 0.0);
}

__global__ void __launch_bounds__(256) eval_detect_update_kernel(const double* __restrict__ part, int chunks, double* __restrict__ hop,
                                                                 const unsigned long long* __restrict__ ctl,
                                                                 double* __restrict__ totals, int Z, int E, int Mv) {
    const size_t items = (size_t)Z * 2 * E * Mv, it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    if (!hop && ctl) {
        const unsigned long long slot = ctl[2] - 1;                              // wraps above every capacity where ctl[2] = 0
        if (slot < ctl[1]) hop = reinterpret_cast<double*>(ctl[0]) + (size_t)slot * items;
    }
    double d = 0.0;
    for (int c = 0; c < chunks; ++c) d += part[(size_t)c * items + it];
    if (hop) hop[it] = d;
    const int m = (int)(it % Mv), j = (int)((it / Mv) % (2 * E)), z = (int)(it / ((size_t)Mv * 2 * E));
    const int kind = j / E, e = j - kind * E;
    double* __restrict__ tz = totals + (((size_t)z * 6 + 3 * kind) * E + e) * Mv + m;
    const size_t plane = (size_t)E * Mv;
    double sum = tz[0], mx = tz[plane], cnt = tz[2 * plane];
    fold_hop(d, sum, mx, cnt);
    tz[0] = sum;
    tz[plane] = mx;
    tz[2 * plane] = cnt;
}

// the hop-batched form: the n hops of part [n][chunks][Z][2 E][Mv] in order, hop i into slot slot0 + i of rec
__global__ void __launch_bounds__(256) eval_detect_update_hops_kernel(const double* __restrict__ part, int chunks, double* __restrict__ rec,
                                                                      long long slot0, double* __restrict__ totals, int Z, int E,
                                                                      int Mv, int n) {
    const size_t items = (size_t)Z * 2 * E * Mv, it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int m = (int)(it % Mv), j = (int)((it / Mv) % (2 * E)), z = (int)(it / ((size_t)Mv * 2 * E));
    const int kind = j / E, e = j - kind * E;
    double* __restrict__ tz = totals + (((size_t)z * 6 + 3 * kind) * E + e) * Mv + m;
    const size_t plane = (size_t)E * Mv;
    double sum = tz[0], mx = tz[plane], cnt = tz[2 * plane];
    for (int i = 0; i < n; ++i) {
        const double* __restrict__ ph = part + (size_t)i * chunks * items + it;
        double d = 0.0;
        for (int c = 0; c < chunks; ++c) d += ph[(size_t)c * items];
        rec[((size_t)slot0 + i) * items + it] = d;
        fold_hop(d, sum, mx, cnt);
    }
    tz[0] = sum;
    tz[plane] = mx;
    tz[2 * plane] = cnt;
}

size_t curve_lds(int K, int C) { return sizeof(double) * ((size_t)K + C); }

}  // namespace

bool apv_eval_detect_size_ok(int N, int Z, int E, int Mv, int C, std::string* why) {
    if (N < 2 || (N & 1) || Z < 1 || Z > 2 || E < 1 || Mv < 1 || C < 1 || C > 512) {
        if (why) *why = "evaluation detectability: even N, Z in 1..2, E and Mv at least 1, 1..512 channels";
        return false;
    }
    if (curve_lds(N / 2 + 1, C) > 64 * 1024) {
        if (why) *why = "evaluation detectability: the bins and channels of one curve do not fit 64 KB of LDS (N/2 + 1 + n_channels <= 8192)";
        return false;
    }
    if ((size_t)Z * E > 65535 || (size_t)Z * (2 * (size_t)E + 1) * Mv > 0x7fffffffull) {
        if (why) *why = "evaluation detectability: at most 65535 (program, rank) pairs and 2^31 - 1 spectra per bin";
        return false;
    }
    return true;
}

int apv_eval_detect_chunks(int N, int Z, int E, int Mv) {
    const long groups = (long)((Mv + ED_T - 1) / ED_T) * Z * E, bins = N / 2;    // bins 1 .. K - 1
    const long want = (ED_FILL + groups - 1) / groups, most = (bins + ED_T - 1) / ED_T;
    return (int)std::max(1L, std::min(std::min(want, most), 64L));
}

hipError_t apv_launch_eval_detect_quiet(int N, int C, const double* G2T, double Cs, double Ca, double Leff, double* quiet, hipStream_t s) {
    if (!apv_eval_detect_size_ok(N, 1, 1, 1, C, nullptr) || !G2T || !quiet) return hipErrorInvalidValue;
    const int K = N / 2 + 1;
    hipLaunchKernelGGL(eval_detect_curve_kernel, dim3(1), dim3(ED_CT), curve_lds(K, C), s, nullptr, 1, 1, K, 1, C, G2T, Cs, Ca, Leff, 0.0,
                       quiet, 1L, nullptr);
    return hipGetLastError();
}

hipError_t apv_launch_eval_detect(const EvalDetectArgs& a, hipStream_t s, std::string* why) {
    if (!apv_eval_detect_size_ok(a.N, a.Z, a.E, a.Mv, a.C, why)) return hipErrorInvalidValue;
    if (!a.spec || !a.G2T || !a.curves || !a.part || !a.totals || (!a.hop && !a.ctl) || (a.Z == 1 && !a.quiet)) {
        if (why) *why = "evaluation detectability: null device pointer";
        return hipErrorInvalidValue;
    }
    const int K = a.N / 2 + 1, chunks = apv_eval_detect_chunks(a.N, a.Z, a.E, a.Mv), kc = (K - 1 + chunks - 1) / chunks;
    const double f = 2.0 / ((double)a.N * (double)a.N);
    const double2* spec = static_cast<const double2*>(a.spec);
    hipLaunchKernelGGL(eval_detect_curve_kernel, dim3((unsigned)(a.Z * a.Mv)), dim3(ED_CT), curve_lds(K, a.C), s, spec, a.Z, a.E, K, a.Mv,
                       a.C, a.G2T, a.Cs, a.Ca, a.Leff, f, a.curves, (long)a.Z * a.Mv, a.hop ? nullptr : a.ctl);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eval_detect_reduce_kernel, dim3((unsigned)((a.Mv + ED_T - 1) / ED_T), (unsigned)(a.Z * a.E), (unsigned)chunks),
                       dim3(256), 0, s, spec, a.curves, a.quiet, a.part, a.Z, a.E, K, a.Mv, kc, f);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t items = (size_t)a.Z * 2 * a.E * a.Mv;
    hipLaunchKernelGGL(eval_detect_update_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a.part, chunks, a.hop, a.ctl,
                       a.totals, a.Z, a.E, a.Mv);
    return hipGetLastError();
}

hipError_t apv_launch_eval_detect_hops(const EvalDetectHopsArgs& a, hipStream_t s, std::string* why) {
    if (!apv_eval_detect_size_ok(a.N, a.Z, a.E, a.Mv, a.C, why)) return hipErrorInvalidValue;
    if (!a.spec || !a.G2T || !a.curves || !a.part || !a.totals || !a.rec || (a.Z == 1 && !a.quiet) || a.slot0 < 0) {
        if (why) *why = "evaluation detectability: null device pointer or a negative slot";
        return hipErrorInvalidValue;
    }
    const long long groups = (a.Mv + ED_T - 1) / ED_T;
    if (a.n < 1 || a.n > 65535 || groups * a.n > 0x7fffffffll) {
        if (why) *why = "evaluation detectability: 1..65535 hops per launch, hops x ceil(Mv / 16) below 2^31";
        return hipErrorInvalidValue;
    }
    const int K = a.N / 2 + 1, chunks = apv_eval_detect_chunks(a.N, a.Z, a.E, a.Mv), kc = (K - 1 + chunks - 1) / chunks;
    const double f = 2.0 / ((double)a.N * (double)a.N);
    const double2* spec = static_cast<const double2*>(a.spec);
    hipLaunchKernelGGL(eval_detect_curve_hops_kernel, dim3((unsigned)(a.Z * a.Mv), (unsigned)a.n), dim3(ED_CT), curve_lds(K, a.C), s, spec,
                       a.Z, a.E, K, a.Mv, a.C, a.G2T, a.Cs, a.Ca, a.Leff, f, a.curves);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(eval_detect_reduce_hops_kernel, dim3((unsigned)(groups * a.n), (unsigned)(a.Z * a.E), (unsigned)chunks), dim3(256),
                       0, s, spec, a.curves, a.quiet, a.part, a.Z, a.E, K, a.Mv, kc, f, (int)groups);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t items = (size_t)a.Z * 2 * a.E * a.Mv;
    hipLaunchKernelGGL(eval_detect_update_hops_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a.part, chunks, a.rec,
                       (long long)a.slot0, a.totals, a.Z, a.E, a.Mv, a.n);
    return hipGetLastError();
}
