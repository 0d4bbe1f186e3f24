// Zero-latency FIR synthesis of the constrained subband stream (apv_stream_set_synthesis(h, APV_SYNTH_FIR)): the J taps that the
// filter-length constraint leaves in "w_time_*" applied to the input signals as plain time-domain FIR filters, in place of the
// output spectra (K3) and the inverse transform with overlap-add (K4).  For hop h, sample t = 0..H-1, n = h H + t, a_t = (t + 1) / H:
//
//   y[z, v][n, l] = (1 - a_t) sum_{j < J} g_{h-1}[z, v, j, l] x_z[n - j]  +  a_t sum_{j < J} g_h[z, v, j, l] x_z[n - j]
//
// a linear cross-fade from the previous hop's taps to this hop's over the hop (g_{-1} = 0: the first hop fades in from silence;
// the hop's last sample takes the new taps alone), and the two target paths are the pure delays x_z[n - modeling_delay] in the
// column of the reference loudspeaker.                                     replaces: nothing in the reference
//
// Per (zone program, rank) this is two implicit-Toeplitz GEMMs with one A operand, (H x J window of the input history) x (J x L
// taps), and a blend.  fir_f64_mfma_kernel (kernels_stream.hip) is the model: the history window of a workgroup's samples sits in
// LDS and is read as the A operand of the 16x16x4 MFMA (lane l: A[i = l & 15][k = l >> 4]) at offset (n0 + i) - (j0 + k); the
// taps stream from memory straight into B operands (lane l: B[k = l >> 4][col = l & 15]: the taps buffer is [nV][J][L], L
// contiguous, so a wave's load is four 16-element runs); the four waves of a workgroup split the taps, and their partial tiles,
// already blended, are summed through LDS in a fixed order (the result does not depend on the launch).  A workgroup owns NT x 16
// samples x 16 loudspeakers of one group; blockIdx.z walks the groups [programs that run: nV][target A][target B], which is the
// order of the stream's result buffer.  The target groups copy: a delay has nothing to round.
//
// A chunk of hops in one launch (FirSynthArgs::n_hops, the chunked whole-signal path): blockIdx.z = hop x group.  Hop i of the
// chunk is the grid of a launch of its own, shifted: its taps lie i hop_taps elements into the chunk's taps buffer and the taps it
// fades from directly in front of them (hop 0: a.prev), its samples i hop_x elements into one linear row per signal, its results
// hop_out bytes behind those of hop i - 1.  No hop reads what another hop of the launch writes; a (hop, group, tile) runs the
// arithmetic of the per-hop launch in the same order, so the bits are the same.
//
// Arithmetic: float64 on v_mfma_f64_16x16x4_f64 unless taps AND samples are float32 (v_mfma_f32_16x16x4_f32).  A dtype="mixed"
// stream (float64 filters, float32 samples) widens the samples when it fills the window and rounds the result once.
//
// Bounds: the window load, the tap loads and the stores are all predicated -- L need not be a multiple of 16, H of the sample
// tile, J of the k-step of 4; nothing is read or written past [J - 1 + H] samples, [nV][J][L] taps and [H][L] results per group.
#include "apv_internal.h"

#include <algorithm>
#include <type_traits>

namespace {

using fs_d4 = __attribute__((ext_vector_type(4))) double;
using fs_f4 = __attribute__((ext_vector_type(4))) float;

constexpr int FS_PT = 16 * 17;                 // one partial tile in LDS: [16 samples][16 loudspeakers], rows padded to 17

template <typename CT> struct FsAcc;
template <> struct FsAcc<double> {
    using V = fs_d4;
    static __device__ __forceinline__ V mfma(double a, double b, V c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    // accumulator element r of lane: sample (lane >> 4) + 4 r, loudspeaker lane & 15
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <> struct FsAcc<float> {
    using V = fs_f4;
    static __device__ __forceinline__ V mfma(float a, float b, V c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    // sample 4 (lane >> 4) + r, loudspeaker lane & 15
    static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

template <typename TT, typename TX, int NT>
__global__ void __launch_bounds__(256) fir_synth_kernel(FirSynthArgs a) {
    using CT = typename std::conditional<std::is_same<TT, float>::value && std::is_same<TX, float>::value, float, double>::type;
    using Acc = FsAcc<CT>;
    using V4 = typename Acc::V;
    extern __shared__ __align__(16) unsigned char fs_lds[];
    CT* xw = reinterpret_cast<CT*>(fs_lds);      // [J - 1 + 16 NT] history window; afterwards [4][NT][FS_PT] partial tiles
    CT* part = xw;
    const int J = a.J, H = a.H, L = a.L;
    const int nfilt = a.nz * a.nV, groups = nfilt + a.n_tgt;
    // a launch of one hop has gridDim.z = groups: hop = 0 and none of the hop strides is multiplied
    const int hop = blockIdx.z / groups, g = blockIdx.z - hop * groups, l0 = blockIdx.y * 16, n0 = blockIdx.x * 16 * NT;
    const bool is_tgt = g >= nfilt;               // uniform per workgroup
    const int z = is_tgt ? 0 : g / a.nV, v = is_tgt ? 0 : g - z * a.nV;
    const int sig = is_tgt ? g - nfilt : a.sig[z];
    const TX* __restrict__ xh = static_cast<const TX*>(a.xhist[sig]) + (size_t)hop * a.hop_x;
    const TX* __restrict__ xp = static_cast<const TX*>(a.xhop[sig]) + (size_t)hop * a.hop_x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, il = lane & 15, kq = lane >> 4;
    // window element i is sample n0 - (J - 1) + i of the hop: the J - 1 samples in front of the hop, the hop, zeros past its end
    for (int i = tid; i < J - 1 + 16 * NT; i += 256) {
        const int q = n0 + i;
        xw[i] = q < J - 1 ? (CT)xh[q] : (q < J - 1 + H ? (CT)xp[q - (J - 1)] : (CT)0);
    }
    __syncthreads();
    TX* __restrict__ out = reinterpret_cast<TX*>(static_cast<char*>(a.out) + (size_t)hop * a.hop_out) + (size_t)g * H * L;
    // the thread that stores sample row nl, loudspeaker column c of a tile: neighbouring threads along the contiguous axis of the result
    const int nl = a.sl == 1 ? tid >> 4 : tid & 15, c = a.sl == 1 ? tid & 15 : tid >> 4;
    if (is_tgt) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + 16 * t + nl, l = l0 + c;
            if (n < H && l < L) out[(size_t)n * a.sn + (size_t)l * a.sl] = l == a.ref ? (TX)xw[J - 1 + 16 * t + nl - a.delay] : (TX)0;
        }
        return;
    }
    // hop i of a chunk fades from the taps of hop i - 1, which lie in front of its own; the chunk's first hop from a.prev
    const TT* __restrict__ gc = static_cast<const TT*>(a.cur[z]) + (size_t)hop * a.hop_taps + (size_t)v * J * L;
    const TT* __restrict__ gp = hop > 0 ? gc - a.hop_taps : static_cast<const TT*>(a.prev[z]) + (size_t)v * J * L;
    const int steps_total = (J + 3) >> 2, spw = (steps_total + 3) >> 2;
    const int s_begin = wave * spw, s_end = min(s_begin + spw, steps_total);
    const int l = l0 + il;
    const bool l_ok = l < L;
    V4 accp[NT], accc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        accp[t] = (V4){0, 0, 0, 0};
        accc[t] = (V4){0, 0, 0, 0};
    }
    constexpr int G = 8;                         // k-steps whose taps are in flight together
    auto load_taps = [&](CT (&dp)[G], CT (&dc)[G], int s0) {
#pragma unroll
        for (int q = 0; q < G; ++q) {
            const int j = 4 * (s0 + q) + kq;
            const bool ok = s0 + q < s_end && j < J && l_ok;
            dp[q] = ok ? (CT)gp[(size_t)j * L + l] : (CT)0;
            dc[q] = ok ? (CT)gc[(size_t)j * L + l] : (CT)0;
        }
    };
    CT bp[G], bc[G], np[G], nc[G];
    load_taps(bp, bc, s_begin);
    for (int s0 = s_begin; s0 < s_end; s0 += G) {
        load_taps(np, nc, s0 + G);                           // past s_end: all zeros, never used
#pragma unroll
        for (int q = 0; q < G; ++q) {
            if (s0 + q >= s_end) break;                      // wave-uniform
            const int wi = J - 1 + il - (4 * (s0 + q) + kq); // below zero only for taps past J, whose B operands are zero
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int wj = wi + 16 * t;
                const CT xa = xw[wj > 0 ? wj : 0];
                accp[t] = Acc::mfma(xa, bp[q], accp[t]);
                accc[t] = Acc::mfma(xa, bc[q], accc[t]);
            }
        }
#pragma unroll
        for (int q = 0; q < G; ++q) {
            bp[q] = np[q];
            bc[q] = nc[q];
        }
    }
    __syncthreads();                                         // every wave is done with the window
    // the wave's share of both sums, blended: y_prev + a (y_cur - y_prev), which returns y_prev itself where the two agree; the
    // hop's last sample is y_cur alone
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = Acc::row(lane, r), n = n0 + 16 * t + row;
            const CT al = (CT)(n + 1) / (CT)H;
            const CT yp = accp[t][r], yc = accc[t][r];
            part[(wave * NT + t) * FS_PT + row * 17 + il] = n + 1 == H ? yc : yp + al * (yc - yp);
        }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int e = t * FS_PT + nl * 17 + c;
        const CT y = ((part[e] + part[NT * FS_PT + e]) + part[2 * NT * FS_PT + e]) + part[3 * NT * FS_PT + e];
        const int n = n0 + 16 * t + nl, lo = l0 + c;
        if (n < H && lo < L) out[(size_t)n * a.sn + (size_t)lo * a.sl] = (TX)y;
    }
}

// behind the synthesis of a hop: the hop's taps become the taps the next hop fades from (blockIdx.y < nz), and the J - 1 newest
// samples of [history | hop] the next hop's history (blockIdx.y - nz = input signal; written to the OTHER history buffer: with
// J - 1 > H source and destination overlap)
template <typename TT, typename TX>
__global__ void __launch_bounds__(256) fir_synth_advance_kernel(FirSynthAdvance a) {
    const int y = blockIdx.y;
    if (y < a.nz) {
        const TT* __restrict__ src = static_cast<const TT*>(a.cur[y]);
        TT* __restrict__ dst = static_cast<TT*>(a.prev[y]);
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < a.n_taps; i += (size_t)gridDim.x * 256) dst[i] = src[i];
        return;
    }
    const int g = y - a.nz, keep = a.J - 1;
    const TX* __restrict__ oh = static_cast<const TX*>(a.old_hist[g]);
    const TX* __restrict__ xp = static_cast<const TX*>(a.xhop[g]);
    TX* __restrict__ nh = static_cast<TX*>(a.new_hist[g]);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < keep; i += gridDim.x * 256) {
        const int q = i + a.H;
        nh[i] = q < keep ? oh[q] : xp[q - keep];
    }
}

// rows[g][i], i < J - 1 + nc H: the head from head[g][head_off + i], the body from the staged hops pin [nc][2][H]
template <typename TX>
__global__ void __launch_bounds__(256) fir_synth_rows_kernel(int J, int H, int nc, const TX* __restrict__ head0, const TX* __restrict__ head1,
                                                             size_t head_off, const TX* __restrict__ pin, TX* __restrict__ row0,
                                                             TX* __restrict__ row1) {
    const int g = blockIdx.y, keep = J - 1;
    const TX* __restrict__ hd = (g ? head1 : head0) + head_off;
    TX* __restrict__ row = g ? row1 : row0;
    const size_t len = (size_t)keep + (size_t)nc * H;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (size_t)gridDim.x * 256) {
        if (i < (size_t)keep) {
            row[i] = hd[i];
        } else {
            const size_t m = i - keep, q = m / H, t = m - q * H;
            row[i] = pin[(q * 2 + g) * H + t];
        }
    }
}

template <typename TT, typename TX>
hipError_t launch_fir_synth(const FirSynthArgs& a, hipStream_t s, std::string* why) {
    using CT = typename std::conditional<std::is_same<TT, float>::value && std::is_same<TX, float>::value, float, double>::type;
    const int groups = a.nz * a.nV + a.n_tgt;
    const int NT = a.H >= 256 ? 4 : 1;           // as K1: four sample tiles per tap load once the hop still fills the chip
    const size_t lds = sizeof(CT) * std::max((size_t)a.J - 1 + 16 * NT, (size_t)4 * NT * FS_PT);
    if (lds > 64 * 1024) {
        if (why) *why = "FIR synthesis: the history window of J - 1 + 64 samples does not fit 64 KB of LDS";
        return hipErrorInvalidValue;
    }
    const dim3 grid((a.H + 16 * NT - 1) / (16 * NT), (a.L + 15) / 16, groups * std::max(a.n_hops, 1));
    if (NT == 4) hipLaunchKernelGGL((fir_synth_kernel<TT, TX, 4>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((fir_synth_kernel<TT, TX, 1>), grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t apv_launch_fir_synthesis(int taps_f64, int x_f64, const FirSynthArgs& a, hipStream_t s, std::string* why) {
    if (a.J < 1 || a.H < 1 || a.L < 1 || a.nV < 1 || a.nz < 0 || a.nz > 2 || (a.n_tgt != 0 && a.n_tgt != 2) ||
        a.nz * a.nV + a.n_tgt < 1 || (long)(a.nz * a.nV + a.n_tgt) * std::max(a.n_hops, 1) > 65535 || !a.out) {
        if (why) *why = "FIR synthesis: J, H, L, nV must be positive, with at most two zone programs and at most 65535 groups x hops";
        return hipErrorInvalidValue;
    }
    if (a.n_tgt && (a.delay < 0 || a.delay >= a.J)) {
        if (why) *why = "FIR synthesis: the target delay must lie inside the J taps";
        return hipErrorInvalidValue;
    }
    if (taps_f64) return x_f64 ? launch_fir_synth<double, double>(a, s, why) : launch_fir_synth<double, float>(a, s, why);
    return x_f64 ? launch_fir_synth<float, double>(a, s, why) : launch_fir_synth<float, float>(a, s, why);
}

hipError_t apv_launch_fir_synth_rows(int x_f64, int J, int H, int nc, const void* const head[2], size_t head_off, const void* pin,
                                     void* const rows[2], hipStream_t s) {
    if (J < 1 || H < 1 || nc < 1) return hipErrorInvalidValue;
    const size_t len = (size_t)J - 1 + (size_t)nc * H;
    const dim3 grid((unsigned)std::min<size_t>((len + 255) / 256, 1024), 2);
    if (x_f64)
        hipLaunchKernelGGL(fir_synth_rows_kernel<double>, grid, dim3(256), 0, s, J, H, nc, (const double*)head[0], (const double*)head[1],
                           head_off, (const double*)pin, (double*)rows[0], (double*)rows[1]);
    else
        hipLaunchKernelGGL(fir_synth_rows_kernel<float>, grid, dim3(256), 0, s, J, H, nc, (const float*)head[0], (const float*)head[1],
                           head_off, (const float*)pin, (float*)rows[0], (float*)rows[1]);
    return hipGetLastError();
}

hipError_t apv_launch_fir_synth_advance(int taps_f64, int x_f64, const FirSynthAdvance& a, hipStream_t s) {
    if (a.nz < 0 || a.nz > 2 || a.J < 1 || a.H < 1) return hipErrorInvalidValue;
    const size_t most = std::max(a.n_taps, (size_t)a.J);
    const dim3 grid((unsigned)std::min<size_t>((most + 255) / 256, 1024), a.nz + 2);
    if (taps_f64) {
        if (x_f64) hipLaunchKernelGGL((fir_synth_advance_kernel<double, double>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((fir_synth_advance_kernel<double, float>), grid, dim3(256), 0, s, a);
    } else {
        if (x_f64) hipLaunchKernelGGL((fir_synth_advance_kernel<float, double>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((fir_synth_advance_kernel<float, float>), grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}
