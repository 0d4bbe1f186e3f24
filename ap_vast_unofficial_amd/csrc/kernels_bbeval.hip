// Evaluation stage of the broadband stream (apv_bb_set_evaluation): what follows the pressure launch of kernels_streameval.hip when
// one launch covers n hops -- a group of apv_bb_process_signal, n = 1 in apv_bb_process_block.  The pressures of a launch are
// p [Z][2 E + 1][n H][Mv] (per zone program: bright of the E evaluated ranks, dark of the E ranks, target), hop i of a set being its
// rows i H .. (i + 1) H - 1.
//
// 1. bbeval_energy_kernel.  Per hop i, program z, energy k of [bright of E ranks | dark | error | target] and microphone m
//
//   e[i][z][k][m] = sum_{t < H} v[i H + t, m]^2,   v = p_bright, p_dark, p_target - p_bright, p_target
//
// into slot slot0 + i of the per-call record [slots][Z][3 E + 1][Mv].  One wavefront owns one (i, z, k) and 16 neighbouring
// microphones: lane = 16 q + c reads microphone c of the rows t = q, q + 4, q + 8, ... in ascending order (a row's 16 doubles are one
// 128-byte run) and the four partial sums of a microphone are combined by the fixed tree (s_0 + s_1) + (s_2 + s_3), over the lanes
// 16 and 32 apart.  So the order of a hop's sum depends on H alone: not on n, not on where the hop stands in the launch, not on Mv,
// not on the grid.  No atomics.
//
// 2. bbeval_advance_kernel.  blockIdx.y = 0: total = total + hop for the n slots in hop order, one thread per element of a slot.
// blockIdx.y = 1 + g: the newest Pv - 1 samples of [history | n H samples] of evaluated group g into the OTHER history buffer
// (Pv - 1 may exceed n H: source and destination would overlap).
//
// Bounds: every load and store is predicated on m < Mv, t < H and the item counts; nothing is read past p, [Pv - 1][L] history
// samples and n H x L emitted samples per group, nothing written past slots slot0 .. slot0 + n - 1, the totals and the history.
#include "apv_internal.h"

#include <algorithm>

namespace {

constexpr int BE_TL = 4;        // rows in flight per wavefront: lanes 16 q + c, q < BE_TL
constexpr int BE_WAVES = 4;     // wavefronts per workgroup

__global__ void __launch_bounds__(64 * BE_WAVES) bbeval_energy_kernel(BbEvalEnergyArgs a) {
    const int H = a.H, Mv = a.Mv, E = a.E, per_z = 3 * E + 1, mt = (Mv + 15) / 16;
    const size_t HM = (size_t)H * Mv, set_stride = (size_t)a.n * HM;
    const long long n_items = (long long)a.n * a.Z * per_z * mt;
    const int lane = threadIdx.x & 63, c = lane & 15, q = lane >> 4;
    const long long item = (long long)blockIdx.x * BE_WAVES + (threadIdx.x >> 6);
    if (item >= n_items) return;                                      // wave-uniform
    const int tile = (int)(item % mt);
    long long r = item / mt;
    const int k = (int)(r % per_z);
    r /= per_z;
    const int z = (int)(r % a.Z), i = (int)(r / a.Z);
    const int m = tile * 16 + c;
    const bool ok = m < Mv;
    const double* __restrict__ pz = a.p + (size_t)z * (2 * E + 1) * set_stride + (size_t)i * HM + (ok ? m : 0);
    const double* __restrict__ pt = pz + (size_t)2 * E * set_stride;  // the program's target pressure
    const bool diff = k >= 2 * E && k < 3 * E;
    const double* __restrict__ pa = k < 2 * E ? pz + (size_t)k * set_stride : (diff ? pz + (size_t)(k - 2 * E) * set_stride : pt);
    double e = 0.0;
    if (ok) {
        if (diff) {
#pragma unroll 4
            for (int t = q; t < H; t += BE_TL) {
                const double v = pt[(size_t)t * Mv] - pa[(size_t)t * Mv];
                e += v * v;
            }
        } else {
#pragma unroll 4
            for (int t = q; t < H; t += BE_TL) {
                const double v = pa[(size_t)t * Mv];
                e += v * v;
            }
        }
    }
    e += __shfl_xor(e, 16);
    e += __shfl_xor(e, 32);
    if (ok && q == 0) a.rec[((size_t)a.slot0 + i) * ((size_t)a.Z * per_z * Mv) + ((size_t)z * per_z + k) * Mv + m] = e;
}

__global__ void __launch_bounds__(256) bbeval_advance_kernel(BbEvalAdvanceArgs a) {
    if (blockIdx.y == 0) {
        const size_t items = (size_t)a.Z * (3 * a.E + 1) * a.Mv;
        const double* __restrict__ rec = a.rec + (size_t)a.slot0 * items;
        for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
            double tot = a.totals[it];
            for (int i = 0; i < a.n; ++i) tot = tot + rec[(size_t)i * items + it];
            a.totals[it] = tot;
        }
        return;
    }
    const int g = blockIdx.y - 1, keep = a.Pv - 1, L = a.L;
    const long long span = (long long)a.n * a.H;                      // samples of the launch
    const double* __restrict__ oh = a.old_hist + (size_t)g * keep * L;
    double* __restrict__ nh = a.new_hist + (size_t)g * keep * L;
    const double* __restrict__ hp = a.hop + (size_t)a.hist_src[g] * a.hop_stride;
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < keep * L; idx += gridDim.x * 256) {
        const int i = idx / L, l = idx - i * L;
        const long long qq = i + span;
        nh[idx] = qq < keep ? oh[(size_t)qq * L + l] : hp[(size_t)(qq - keep) * a.sn + (size_t)l * a.sl];
    }
}

}  // namespace

bool apv_bbeval_sizes_ok(int Z, int E, int H, int Mv, int n, std::string* why) {
    if (Z < 1 || Z > 2 || E < 1 || H < 1 || Mv < 1 || n < 1) {
        if (why) *why = "evaluation energies: Z must be 1 or 2, and E, H, Mv and the number of hops at least 1";
        return false;
    }
    const unsigned long long items = (unsigned long long)n * Z * (3ull * E + 1) * ((Mv + 15ull) / 16);
    if ((unsigned long long)n * H > 0x7fffffffull || (items + BE_WAVES - 1) / BE_WAVES > 0x7fffffffull) {
        if (why) *why = "evaluation energies: n_hops x H and the launch's (hop, program, energy, 16 microphones) items must stay below 2^31";
        return false;
    }
    return true;
}

hipError_t apv_launch_bbeval_energies(const BbEvalEnergyArgs& a, hipStream_t s, std::string* why) {
    if (!apv_bbeval_sizes_ok(a.Z, a.E, a.H, a.Mv, a.n, why)) return hipErrorInvalidValue;
    if (!a.p || !a.rec || a.slot0 < 0) {
        if (why) *why = "evaluation energies: null device pointer or negative slot";
        return hipErrorInvalidValue;
    }
    const unsigned long long items = (unsigned long long)a.n * a.Z * (3ull * a.E + 1) * ((a.Mv + 15ull) / 16);
    hipLaunchKernelGGL(bbeval_energy_kernel, dim3((unsigned)((items + BE_WAVES - 1) / BE_WAVES)), dim3(64 * BE_WAVES), 0, s, a);
    return hipGetLastError();
}

hipError_t apv_launch_bbeval_advance(const BbEvalAdvanceArgs& a, hipStream_t s) {
    if (a.Z < 1 || a.Z > 2 || a.E < 1 || a.H < 1 || a.Mv < 1 || a.n < 1 || a.Pv < 1 || a.L < 1 || a.n_hist < 0 || a.n_hist > 65534 ||
        a.slot0 < 0 || !a.rec || !a.totals)
        return hipErrorInvalidValue;
    const bool hist = a.Pv > 1 && a.n_hist > 0;
    if (hist && (!a.old_hist || !a.new_hist || !a.hop || !a.hist_src)) return hipErrorInvalidValue;
    const size_t items = (size_t)a.Z * (3 * a.E + 1) * a.Mv, hl = ((size_t)a.Pv - 1) * a.L;
    if (hl > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)std::min<size_t>((std::max(items, hist ? hl : 0) + 255) / 256, 1024), hist ? 1 + a.n_hist : 1);
    hipLaunchKernelGGL(bbeval_advance_kernel, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
