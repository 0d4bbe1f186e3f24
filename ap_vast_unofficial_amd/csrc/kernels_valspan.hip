// Rank choice per bin by the contrast at validation microphones (apv_stream_set_validation_span, apv_validation_span; DESIGN.md
// 4.27).  The contrast is that of Matlab/main.m:120-130, the energy at the microphones of the program's own zone over the energy
// at those of the other zone, predicted per bin from the static transfer functions G [K][Mv][L] of the validation responses (the
// program's signal is a common factor of both energies and cancels).  The filters of a hop lie bin-major, [K][nV][L], slots in
// ascending rank.  Per zone program, bin k and slot t, float64 throughout (complex64 filters are widened exactly):
//
//   bright_t = sum_m |sum_l G_own[k, m, l]   W[k, t, l]|^2
//   dark_t   = sum_m |sum_l G_other[k, m, l] W[k, t, l]|^2
//   slot t' is admissible          if both energies are finite and bright_t' >= phi dark_t' (phi [K] linear, no division)
//   src_t = the largest admissible t' <= t
//   src_t = the running best of the slots t' <= t with finite energies, where none of them is admissible: the scan goes up from
//           slot 0 and takes t' when it is BETTER than the best so far -- better(a, b): a is not 0/0 and b is, or neither is and
//           bright_a dark_b > bright_b dark_a (cross-multiplied, each product rounded once).  So a tie keeps the smaller slot, a
//           slot with dark = 0 < bright beats every finite ratio, and 0/0 ranks lowest
//   src_t = -1                     no slot t' <= t has finite energies: slot t is left as it is
//   phi = 0                        no floor in the bin: src_t = t (-1 where the slot's energies are not finite), nothing is stored
//   slot t becomes a bit copy of slot src_t
//
// In place.  Sources are never themselves replaced: if s = src_t is admissible, the largest admissible slot at or below s is s;
// if s is the running best after slot t of a prefix with no admissible slot, then the prefix up to s has none either and the
// scan, which is the same scan, stood at s after slot s (it took s there and nothing later up to t beat it).  Either way
// src_s = s, so no slot that is read by a copy is written by one, whatever order the copies run in.
//
// One workgroup of four wavefronts owns a bin and serves both zone programs, so the bin's two banks and two filter sets come from
// memory once per hop (the second product that reads them finds them in cache).  The products are (Mv x L) * (L x nV), complex:
//
//   MFMA (Mv >= 16 and nV >= 16: a 16 x 16 tile of microphones x slots fills): a wavefront takes (program, bank, 16 slots) and
//     walks the microphones 16 at a time; per step of four loudspeakers four v_mfma_f64_16x16x4_f64 add Gr Wr, -Gi Wi to the real
//     and Gr Wi, Gi Wr to the imaginary accumulator (A: lane holds G[m0 + (lane & 15)][l0 + (lane >> 4)], B: W[t0 + (lane &
//     15)][l0 + (lane >> 4)], D: slot lane & 15, microphone (lane >> 4) + 4 r).  Elements beyond Mv, nV, L are loaded as zeros
//     (predicated), and zero rows add exact zeros.  A lane squares and adds its four microphones in the order of r, the four lane
//     groups are added by two butterflies, and the tiles of 16 microphones are added in ascending order.
//   FMA (otherwise): a wavefront takes (program, bank, slot); lane j accumulates microphones j, j + 64, ... in that order, each
//     a complex dot product over l = 0 .. L - 1 in order, then a six-step butterfly adds the lanes.
//
// No atomics; the order of every sum is a function of (Mv, nV, L) alone, so two launches on the same inputs agree bit for bit.
// The energies (at most 2 x 2 x 128) and sources live in LDS; every global access is predicated by K (the grid), L, Mv and nV,
// and nothing but W, the outputs and LDS is written.  emit = 0: the outputs are not written (W still is).
#include "apv_internal.h"
#include "stft_fft.h"

namespace {

typedef double vs_d4 __attribute__((ext_vector_type(4)));

template <typename T>
struct ValSpanJobs {
    C2<T>* w[2];                    // [K][nV][L] per zone program of the launch, replaced in place
    const C2<double>* g[2][2];      // [program][0: the bank of its own zone (bright), 1: of the other zone (dark)], [K][Mv][L]
    const double* phi[2];           // [K]
    double* energy[2][2];           // [program][bright, dark], [K][nV]
    int32_t* src[2];                // [K][nV]
    int zones, emit;
};

__device__ __forceinline__ bool vs_finite(double e) { return e - e == 0.0; }

// slot (b1, d1) ranks above slot (b2, d2); both have finite energies (>= 0)
__device__ __forceinline__ bool vs_better(double b1, double d1, double b2, double d2) {
    const bool n1 = b1 != 0.0 || d1 != 0.0, n2 = b2 != 0.0 || d2 != 0.0;       // not 0/0
    if (n1 != n2) return n1;
    if (!n1) return false;
    return __dmul_rn(b1, d2) > __dmul_rn(b2, d1);
}

template <typename T, bool MFMA>
__global__ void __launch_bounds__(256) validation_span_kernel(ValSpanJobs<T> jobs, int nV, int L, int Mv) {
    __shared__ double s_e[2][2][APV_VALSPAN_MAX_SLOTS];
    __shared__ int s_src[2][APV_VALSPAN_MAX_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, k = blockIdx.x;

    // the energies
    if (MFMA) {
        const int tiles = (nV + 15) >> 4, items = jobs.zones * 2 * tiles;
        const int c = lane & 15, q = lane >> 4;
        for (int it = wave; it < items; it += 4) {
            const int z = it / (2 * tiles), r = it - z * 2 * tiles, b = r / tiles, t = (r - b * tiles) * 16 + c;
            const C2<T>* __restrict__ W = jobs.w[z] + (size_t)k * nV * L;
            const C2<double>* __restrict__ G = jobs.g[z][b] + (size_t)k * Mv * L;
            double e = 0.0;
            for (int m0 = 0; m0 < Mv; m0 += 16) {
                const int m = m0 + c;
                vs_d4 are = {0.0, 0.0, 0.0, 0.0}, aim = {0.0, 0.0, 0.0, 0.0};
                for (int l0 = 0; l0 < L; l0 += 4) {
                    const int l = l0 + q;
                    double gr = 0.0, gi = 0.0, wr = 0.0, wi = 0.0;
                    if (l < L && m < Mv) {
                        const C2<double> g = G[(size_t)m * L + l];
                        gr = g.x; gi = g.y;
                    }
                    if (l < L && t < nV) {
                        const C2<T> x = W[(size_t)t * L + l];
                        wr = (double)x.x; wi = (double)x.y;
                    }
                    are = __builtin_amdgcn_mfma_f64_16x16x4f64(gr, wr, are, 0, 0, 0);
                    are = __builtin_amdgcn_mfma_f64_16x16x4f64(-gi, wi, are, 0, 0, 0);
                    aim = __builtin_amdgcn_mfma_f64_16x16x4f64(gr, wi, aim, 0, 0, 0);
                    aim = __builtin_amdgcn_mfma_f64_16x16x4f64(gi, wr, aim, 0, 0, 0);
                }
                double p = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) p += are[i] * are[i] + aim[i] * aim[i];
                p += __shfl_xor(p, 16, 64);
                p += __shfl_xor(p, 32, 64);
                e += p;
            }
            if (q == 0 && t < nV) s_e[z][b][t] = e;
        }
    } else {
        const int items = jobs.zones * 2 * nV;
        for (int it = wave; it < items; it += 4) {
            const int z = it / (2 * nV), r = it - z * 2 * nV, b = r / nV, t = r - b * nV;
            const C2<T>* __restrict__ W = jobs.w[z] + ((size_t)k * nV + t) * L;
            const C2<double>* __restrict__ G = jobs.g[z][b] + (size_t)k * Mv * L;
            double e = 0.0;
            for (int m = lane; m < Mv; m += 64) {
                double re = 0.0, im = 0.0;
                for (int l = 0; l < L; ++l) {
                    const C2<double> g = G[(size_t)m * L + l];
                    const C2<T> x = W[l];
                    const double wr = (double)x.x, wi = (double)x.y;
                    re += g.x * wr - g.y * wi;
                    im += g.x * wi + g.y * wr;
                }
                e += re * re + im * im;
            }
            for (int o = 32; o >= 1; o >>= 1) e += __shfl_xor(e, o, 64);
            if (lane == 0) s_e[z][b][t] = e;
        }
    }
    __syncthreads();            // every read of W by the products lies before it

    // the source of every slot
    bool changes = false;
    for (int i = tid; i < jobs.zones * nV; i += 256) {
        const int z = i / nV, t = i - z * nV;
        const double phi = jobs.phi[z][k];
        int last = -1, best = -1;
        for (int tp = 0; tp <= t; ++tp) {
            const double b = s_e[z][0][tp], d = s_e[z][1][tp];
            if (!(vs_finite(b) && vs_finite(d))) continue;
            if (b >= __dmul_rn(phi, d)) last = tp;
            if (best < 0 || vs_better(b, d, s_e[z][0][best], s_e[z][1][best])) best = tp;
        }
        int s = last >= 0 ? last : best;
        if (phi == 0.0) s = (vs_finite(s_e[z][0][t]) && vs_finite(s_e[z][1][t])) ? t : -1;
        s_src[z][t] = s;
        changes = changes || (s >= 0 && s != t);
    }
    const int any = __syncthreads_or(changes);

    if (jobs.emit)
        for (int i = tid; i < jobs.zones * nV; i += 256) {
            const int z = i / nV, t = i - z * nV;
            const size_t o = (size_t)k * nV + t;
            jobs.energy[z][0][o] = s_e[z][0][t];
            jobs.energy[z][1][o] = s_e[z][1][t];
            jobs.src[z][o] = s_src[z][t];
        }
    if (!any) return;

    // the copies; a source is its own source (see the file header), so no slot read here is written here
    for (int it = wave; it < jobs.zones * nV; it += 4) {
        const int z = it / nV, t = it - z * nV, s = s_src[z][t];
        if (s < 0 || s == t) continue;
        C2<T>* W = jobs.w[z] + (size_t)k * nV * L;
        for (int l = lane; l < L; l += 64) W[(size_t)t * L + l] = W[(size_t)s * L + l];
    }
}

template <typename T>
hipError_t launch_valspan(int K, int nV, int L, int Mv, const ValSpanArgs& a, hipStream_t s) {
    ValSpanJobs<T> jobs{};
    jobs.zones = a.zones;
    jobs.emit = a.emit;
    for (int z = 0; z < a.zones; ++z) {
        jobs.w[z] = (C2<T>*)a.w[z];
        jobs.g[z][0] = (const C2<double>*)a.g_bright[z];
        jobs.g[z][1] = (const C2<double>*)a.g_dark[z];
        jobs.phi[z] = a.phi[z];
        jobs.energy[z][0] = a.bright[z];
        jobs.energy[z][1] = a.dark[z];
        jobs.src[z] = a.src[z];
    }
    if (Mv >= 16 && nV >= 16) hipLaunchKernelGGL((validation_span_kernel<T, true>), dim3(K), dim3(256), 0, s, jobs, nV, L, Mv);
    else hipLaunchKernelGGL((validation_span_kernel<T, false>), dim3(K), dim3(256), 0, s, jobs, nV, L, Mv);
    return hipGetLastError();
}

}  // namespace

hipError_t apv_launch_validation_span(int c128, int K, int nV, int L, int Mv, const ValSpanArgs& a, hipStream_t s, std::string* why) {
    if (K < 1 || nV < 1 || nV > APV_VALSPAN_MAX_SLOTS || L < 1 || L > APV_MAX_SRCS || Mv < 1 || a.zones < 1 || a.zones > 2) {
        if (why) *why = "validation span: K >= 1, 1 <= nV <= 128, 1 <= L <= 128, Mv >= 1, one or two zone programs";
        return hipErrorInvalidValue;
    }
    for (int z = 0; z < a.zones; ++z)
        if (!a.w[z] || !a.g_bright[z] || !a.g_dark[z] || !a.phi[z] || (a.emit && (!a.bright[z] || !a.dark[z] || !a.src[z]))) {
            if (why) *why = "validation span: null filters, transfer functions, floor table or outputs";
            return hipErrorInvalidValue;
        }
    return c128 ? launch_valspan<double>(K, nV, L, Mv, a, s) : launch_valspan<float>(K, nV, L, Mv, a, s);
}
