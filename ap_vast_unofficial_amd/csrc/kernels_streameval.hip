// Evaluation stage of the subband stream (apv_stream_set_evaluation): the hop's own drive signals filtered through the responses to
// validation microphones, behind the synthesis and in front of the copy back.  Per pressure set (source group g of the hop's
// result buffer, response bank rv [Pv][L][Mv]) and absolute sample n, y zero before the first hop:
//
//   p[set][n, m] = sum_l sum_{j < Pv} rv[j, l, m] y[g][n - j, l]                replaces: Matlab/predictPressure.m:12-16, hop by hop
//
// 1. eval_pressure_kernel.  An implicit-Toeplitz GEMM per set, (H x L Pv window of the group's samples) x (L Pv x Mv responses), on
// v_mfma_f64_16x16x4_f64; fir_f64_mfma_kernel (kernels_stream.hip) and fir_synth_kernel (kernels_firsynth.hip) are the models.  A
// workgroup owns NT x 16 samples x 16 microphones of one set.  The samples of LS loudspeakers -- the Pv - 1 in front of the tile
// (from the history buffer while they precede the hop, then from the hop's result buffer, read through strides in whichever layout
// the stream emits) and the tile itself -- are staged in LDS, one row of W = Pv - 1 + 16 NT doubles per loudspeaker, float32
// samples widened as the row is filled; LS is as many rows as the LDS budget holds, and the loudspeakers go through in passes of
// LS.  Lane l reads its A operand A[i = l & 15][k = l >> 4] at row offset (Pv - 1 + i) - (j0 + k) and loads its B operand
// B[k = l >> 4][m = l & 15] straight from the bank (Mv contiguous: four 16-element runs per wave).  The four waves split the taps j
// (the same split whatever H, L or LS are) and walk the loudspeakers in ascending order; their partial tiles are summed through LDS
// in wave order.  So the bits of a sample depend on (Pv, L) and the data alone, not on the launch.
//
// 2. eval_advance_kernel.  blockIdx.y = 0: the four energies of the hop per microphone, one thread per (energy, microphone) summing
// the hop's samples in ascending order (no atomics), written to the slot of the per-call record that the control words name and
// added to the totals, total = total + hop.  blockIdx.y = 1 + history slot: the newest Pv - 1 samples of [history | hop] of every
// evaluated group into the OTHER history buffer (with Pv - 1 > H source and destination would overlap).
//
// The control words ctl[4] = {address of the record, slots it holds, slot counter of parity 0, of parity 1}: a hop of parity c (the
// stream's history parity, part of the period of the captured hop graphs) reads counter c and leaves counter + 1 in counter c ^ 1,
// which no thread of that launch reads.  The host resets the counter the next hop reads at the start of a call, and rewrites the
// first two words when the record grows, so the captured graphs never hold the record's address.
//
// Bounds: the window fill, the bank loads and the stores are predicated: H, L, Mv, Pv need not be multiples of anything; nothing
// is read past [Pv - 1][L] history samples, H x L hop samples and [Pv][L][Mv] responses, nothing written past [sets][H][Mv]
// pressures, the record's slots and the totals.
#include "apv_internal.h"

#include <algorithm>

namespace {

using ev_d4 = __attribute__((ext_vector_type(4))) double;

constexpr int EV_PT = 16 * 17;                 // one partial tile in LDS: [16 samples][16 microphones], rows padded to 17
constexpr size_t EV_LDS_MAX = 160 * 1024;      // LDS of a CU: the most one workgroup can be given

template <typename TX, int NT>
__global__ void __launch_bounds__(256) eval_pressure_kernel(EvalPressureArgs a, int LS, int W) {
    extern __shared__ __align__(16) unsigned char ev_lds[];
    double* xw = reinterpret_cast<double*>(ev_lds);      // [LS][W] sample rows; afterwards [4][NT][EV_PT] partial tiles
    double* part = xw;
    const int Pv = a.Pv, H = a.H, L = a.L, Mv = a.Mv, keep = a.Pv - 1;
    const int set = blockIdx.z, m0 = blockIdx.y * 16, n0 = blockIdx.x * 16 * NT;
    int src = set, hs = set, ri = 0;
    if (a.map) {
        src = a.map[4 * set];
        hs = a.map[4 * set + 1];
        ri = a.map[4 * set + 2];
    }
    const TX* __restrict__ hh = static_cast<const TX*>(a.hist) + (size_t)hs * a.hist_stride;
    const TX* __restrict__ hp = static_cast<const TX*>(a.hop) + (size_t)src * a.hop_stride;
    const double* __restrict__ rv = a.rv[ri];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, il = lane & 15, kq = lane >> 4;
    const int steps_total = (Pv + 3) >> 2, spw = (steps_total + 3) >> 2;
    const int s_begin = wave * spw, s_end = min(s_begin + spw, steps_total);
    const int m = m0 + il;
    const bool m_ok = m < Mv;
    const size_t tap_stride = (size_t)L * Mv;
    ev_d4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (ev_d4){0, 0, 0, 0};
    constexpr int G = 8;                         // k-steps whose responses are in flight together
    for (int lb = 0; lb < L; lb += LS) {
        const int nl = min(LS, L - lb);
        __syncthreads();                         // every wave is done with the rows of the pass before
        // row element i is sample n0 - (Pv - 1) + i of the hop: history while it precedes the hop, zeros past the hop's end
        for (int idx = tid; idx < nl * W; idx += 256) {
            const int i = idx / nl, ll = idx - i * nl, q = n0 + i, l = lb + ll;
            double x = 0.0;
            if (q < keep) x = (double)hh[(size_t)q * L + l];
            else if (q - keep < H) x = (double)hp[(size_t)(q - keep) * a.sn + (size_t)l * a.sl];
            xw[ll * W + i] = x;
        }
        __syncthreads();
        for (int ll = 0; ll < nl; ++ll) {
            const double* xr = xw + ll * W;
            const double* __restrict__ rl = rv + (size_t)(lb + ll) * Mv + m;
            for (int s0 = s_begin; s0 < s_end; s0 += G) {
                double b[G];
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    const int j = 4 * (s0 + q) + kq;
                    const bool ok = s0 + q < s_end && j < Pv && m_ok;
                    b[q] = ok ? rl[(size_t)j * tap_stride] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < G; ++q) {
                    if (s0 + q >= s_end) break;                       // wave-uniform
                    const int wi = keep + il - (4 * (s0 + q) + kq);   // below zero only for taps past Pv, whose B operands are zero
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const int wj = wi + 16 * t;
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(xr[wj > 0 ? wj : 0], b[q], acc[t], 0, 0, 0);
                    }
                }
            }
        }
    }
    __syncthreads();                                                  // every wave is done with the rows
    // accumulator element r of a lane: sample (lane >> 4) + 4 r, microphone lane & 15
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(wave * NT + t) * EV_PT + (kq + 4 * r) * 17 + il] = acc[t][r];
    __syncthreads();
    double* __restrict__ out = a.p + (size_t)set * H * Mv;
    const int nl = tid >> 4, c = tid & 15;                            // neighbouring threads along the microphones
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int e = t * EV_PT + nl * 17 + c;
        const double y = ((part[e] + part[NT * EV_PT + e]) + part[2 * NT * EV_PT + e]) + part[3 * NT * EV_PT + e];
        const int n = n0 + 16 * t + nl, mo = m0 + c;
        if (n < H && mo < Mv) out[(size_t)n * Mv + mo] = y;
    }
}

template <typename TX>
__global__ void __launch_bounds__(256) eval_advance_kernel(EvalAdvanceArgs a) {
    const int H = a.H, Mv = a.Mv, E = a.E;
    if (blockIdx.y == 0) {
        const int per_z = 3 * E + 1, items = a.Z * per_z * Mv;
        const unsigned long long slot = a.ctl[2 + a.par], cap = a.ctl[1];
        double* __restrict__ rec = reinterpret_cast<double*>(a.ctl[0]);
        for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
            const int m = it % Mv, zk = it / Mv, z = zk / per_z, k = zk - z * per_z;
            const double* __restrict__ pz = a.p + (size_t)z * (2 * E + 1) * H * Mv + m;
            const double* __restrict__ pt = pz + (size_t)2 * E * H * Mv;            // the program's target pressure
            const double* __restrict__ pa = k < 2 * E ? pz + (size_t)k * H * Mv : (k < 3 * E ? pz + (size_t)(k - 2 * E) * H * Mv : pt);
            const bool diff = k >= 2 * E && k < 3 * E;
            double e = 0.0;
            for (int n = 0; n < H; ++n) {
                const double v = diff ? pt[(size_t)n * Mv] - pa[(size_t)n * Mv] : pa[(size_t)n * Mv];
                e += v * v;
            }
            if (slot < cap) rec[(size_t)slot * items + it] = e;
            a.totals[it] = a.totals[it] + e;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) a.ctl[2 + (a.par ^ 1)] = slot + 1;
        return;
    }
    const int g = blockIdx.y - 1, keep = a.Pv - 1, L = a.L;
    const TX* __restrict__ oh = static_cast<const TX*>(a.old_hist) + (size_t)g * keep * L;
    TX* __restrict__ nh = static_cast<TX*>(a.new_hist) + (size_t)g * keep * L;
    const TX* __restrict__ hp = static_cast<const TX*>(a.hop) + (size_t)a.hist_src[g] * a.hop_stride;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < keep * L; idx += gridDim.x * 256) {
        const int i = idx / L, l = idx - i * L, q = i + H;
        nh[idx] = q < keep ? oh[(size_t)q * L + l] : hp[(size_t)(q - keep) * a.sn + (size_t)l * a.sl];
    }
}

// sample tiles per workgroup and loudspeaker rows per pass for (Pv, H, L); false: one row does not fit LDS
bool eval_geometry(int Pv, int H, int L, int* NT, int* LS, size_t* lds) {
    int nt = H >= 256 ? 4 : 1;                   // as K1 and the FIR synthesis: four sample tiles per response load once the hop fills the chip
    size_t row = sizeof(double) * ((size_t)Pv - 1 + 16 * nt);
    if (row > EV_LDS_MAX) {
        nt = 1;
        row = sizeof(double) * ((size_t)Pv - 1 + 16);
    }
    if (row > EV_LDS_MAX) return false;
    const size_t budget = row <= 32 * 1024 ? 32 * 1024 : (row <= 64 * 1024 ? 64 * 1024 : EV_LDS_MAX);
    const int ls = (int)std::min<size_t>((size_t)L, budget / row);
    *NT = nt;
    *LS = ls;
    *lds = std::max(row * ls, sizeof(double) * 4 * nt * EV_PT);
    return true;
}

template <typename TX, int NT>
hipError_t eval_attr(size_t lds) {
    static std::atomic<unsigned long long> done{0};
    if (lds <= 64 * 1024) return hipSuccess;
    // (the attribute is raised to the CU's whole LDS once: a later launch of the same instantiation may need more than this one)
    return apv_set_max_dynamic_lds(reinterpret_cast<const void*>(&eval_pressure_kernel<TX, NT>), (int)EV_LDS_MAX, done);
}

template <typename TX>
hipError_t launch_eval_pressure(const EvalPressureArgs& a, hipStream_t s, bool attr_only) {
    int NT, LS;
    size_t lds;
    if (!eval_geometry(a.Pv, a.H, a.L, &NT, &LS, &lds)) return hipErrorInvalidValue;
    const hipError_t e = NT == 4 ? eval_attr<TX, 4>(lds) : eval_attr<TX, 1>(lds);
    if (e != hipSuccess || attr_only) return e;
    const dim3 grid((a.H + 16 * NT - 1) / (16 * NT), (a.Mv + 15) / 16, a.n_sets);
    const int W = a.Pv - 1 + 16 * NT;
    if (NT == 4) hipLaunchKernelGGL((eval_pressure_kernel<TX, 4>), grid, dim3(256), lds, s, a, LS, W);
    else hipLaunchKernelGGL((eval_pressure_kernel<TX, 1>), grid, dim3(256), lds, s, a, LS, W);
    return hipGetLastError();
}

bool eval_sizes_ok(int n_sets, int Pv, int H, int L, int Mv, std::string* why) {
    if (Pv < 1 || H < 1 || L < 1 || Mv < 1 || n_sets < 1 || n_sets > 65535 || (Mv + 15) / 16 > 65535) {
        if (why) *why = "evaluation: Pv, H, L, Mv must be positive, with at most 65535 pressure sets and 16 x 65535 microphones";
        return false;
    }
    if (!apv_eval_pressure_fits(Pv)) {
        if (why) *why = "evaluation: one loudspeaker's window of Pv - 1 + 16 float64 samples does not fit 160 KB of LDS (Pv <= 20465)";
        return false;
    }
    return true;
}

}  // namespace

bool apv_eval_pressure_fits(int Pv) { return Pv >= 1 && sizeof(double) * ((size_t)Pv - 1 + 16) <= EV_LDS_MAX; }

hipError_t apv_eval_pressure_prepare(int x_f64, int Pv, int H, int L) {
    EvalPressureArgs a{};
    a.Pv = Pv; a.H = H; a.L = L;
    return x_f64 ? launch_eval_pressure<double>(a, nullptr, true) : launch_eval_pressure<float>(a, nullptr, true);
}

hipError_t apv_launch_eval_pressure(int x_f64, const EvalPressureArgs& a, hipStream_t s, std::string* why) {
    if (!eval_sizes_ok(a.n_sets, a.Pv, a.H, a.L, a.Mv, why)) return hipErrorInvalidValue;
    if (!a.hop || !a.p || !a.rv[0] || (a.Pv > 1 && !a.hist)) {
        if (why) *why = "evaluation: null device pointer";
        return hipErrorInvalidValue;
    }
    return x_f64 ? launch_eval_pressure<double>(a, s, false) : launch_eval_pressure<float>(a, s, false);
}

hipError_t apv_launch_eval_advance(int x_f64, const EvalAdvanceArgs& a, hipStream_t s) {
    if (a.Z < 1 || a.Z > 2 || a.E < 1 || a.H < 1 || a.Mv < 1 || a.Pv < 1 || a.L < 1 || a.n_hist < 1 || a.n_hist > 65534 || (a.par & ~1))
        return hipErrorInvalidValue;
    const size_t items = (size_t)a.Z * (3 * a.E + 1) * a.Mv, hist = ((size_t)a.Pv - 1) * a.L;
    const dim3 grid((unsigned)std::min<size_t>((std::max(items, hist) + 255) / 256, 1024), a.Pv > 1 ? 1 + a.n_hist : 1);
    if (x_f64) hipLaunchKernelGGL(eval_advance_kernel<double>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(eval_advance_kernel<float>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
