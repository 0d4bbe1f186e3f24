// Array-effort limit of the subband filters (apv_stream_set_effort_limit, apv_limit_effort).  The filters of a
// hop lie bin-major, [K][nV][L]; output slot t of bin k is the filter of (at most) rank ranks[t].  With e_t = sum_l |W[k, t, l]|^2
// and the bin's limit E (linear, +inf: none):
//
//   slot t is admissible           if e_t is finite and e_t <= E
//   src_t = the largest admissible t' <= t
//   src_t = t                      the slot is not written
//   src_t < t                      slot t becomes a bit copy of slot src_t
//   no src_t, e_t finite           slot t becomes W[k, t, :] * sqrt(E / e_t)   (gain in float64, product rounded once)
//   e_t not finite                 the slot is left as it is (it has no source and is none)
//
// Admissible slots never change and are the only sources, so the stage works in place.
//
// One wavefront per (bin, zone program, hop): blockIdx.x = bin, blockIdx.z = hop x zone program, hop i's filters hop_w elements
// behind those of hop i - 1 (a launch of one hop multiplies it by hop index 0).  A group of G = min(64, next power of two >= L)
// lanes takes one slot, 64 / G slots at a time; lane j of the group loads loudspeakers j, j + G, ... (neighbouring lanes touch
// neighbouring elements) and adds their |.|^2 in float64 in that order, then the group adds its lanes in a butterfly: the order
// of the sum is a function of L alone.  The e_t (at most 128) and src_t live in LDS; a bin (256 KB at 128 x 128 complex128) does
// not, so the second pass reads the filters again, from L2.  A bin wholly within its limit stores nothing but its outputs.
//
// Outputs, written by the hop the launch names (emit_hop; EFFORT_EMIT_ALL: every hop, hop i's hop_bins bins behind those of hop
// i - 1; EFFORT_EMIT_NONE: no hop): effort [K][nV] = the e_t before the stage; src [K] = src of the top slot, its own index where
// it was scaled, -1 where its effort was not finite; gain [K] = the gain of the top slot (1 unless scaled).
#include "apv_internal.h"
#include "stft_fft.h"

namespace {

template <typename T>
struct EffortJobs {
    C2<T>* w[2];              // [K][nV][L] per zone program of the launch, limited in place
    const double* limit[2];   // [K]
    double* effort[2];        // [K][nV]
    int32_t* src[2];          // [K]
    double* gain[2];          // [K]
    int zones;                // blockIdx.z = hop * zones + zone program
    int emit_hop;
    size_t hop_w;             // elements from one hop's filters to the next hop's
    size_t hop_bins;          // bins from one hop's outputs to the next hop's (EFFORT_EMIT_ALL)
};

__device__ __forceinline__ bool effort_finite(double e) { return e - e == 0.0; }

template <typename T>
__global__ void __launch_bounds__(64) limit_effort_kernel(EffortJobs<T> jobs, int nV, int L, int gsh) {
    __shared__ double s_e[APV_EFFORT_MAX_SLOTS];
    __shared__ int s_src[APV_EFFORT_MAX_SLOTS];
    const int lane = threadIdx.x, k = blockIdx.x;
    const int hop = blockIdx.z / jobs.zones, zone = blockIdx.z - hop * jobs.zones;
    const int G = 1 << gsh, S = 64 >> gsh, g = lane >> gsh, j = lane & (G - 1);
    C2<T>* __restrict__ W = jobs.w[zone] + (size_t)hop * jobs.hop_w + (size_t)k * nV * L;
    const double E = jobs.limit[zone][k];

    // pass 1: the efforts
    for (int t0 = 0; t0 < nV; t0 += S) {
        const int t = t0 + g;
        double a = 0.0;
        if (t < nV)
            for (int l = j; l < L; l += G) {
                const C2<T> x = W[(size_t)t * L + l];
                const double re = (double)x.x, im = (double)x.y;
                a += re * re + im * im;
            }
        for (int o = G >> 1; o >= 1; o >>= 1) a += __shfl_xor(a, o, 64);
        if (j == 0 && t < nV) s_e[t] = a;
    }
    __syncthreads();
    // the source of every slot: the nearest admissible slot at or below it
    bool changes = false;
    for (int t = lane; t < nV; t += 64) {
        const bool fin = effort_finite(s_e[t]);
        int s = fin ? t : -1;                      // a slot whose effort is not finite has no source: it is left as it is
        while (s >= 0 && !(effort_finite(s_e[s]) && s_e[s] <= E)) --s;
        s_src[t] = s;
        changes = changes || (s != t && fin);
    }
    const int any = __syncthreads_or(changes);

    if (jobs.emit_hop == hop || jobs.emit_hop == EFFORT_EMIT_ALL) {
        const size_t ob = (size_t)hop * jobs.hop_bins + k;
        for (int t = lane; t < nV; t += 64) jobs.effort[zone][ob * nV + t] = s_e[t];
        if (lane == 0) {
            const int top = nV - 1, s = s_src[top];
            const double e = s_e[top];
            const bool scaled = s < 0 && effort_finite(e);
            jobs.src[zone][ob] = s >= 0 ? s : (scaled ? top : -1);
            jobs.gain[zone][ob] = scaled ? sqrt(E / e) : 1.0;
        }
    }
    if (!any) return;

    // pass 2: copies and scalings; sources are admissible slots, which no lane writes
    for (int t0 = 0; t0 < nV; t0 += S) {
        const int t = t0 + g;
        if (t >= nV) continue;
        const int s = s_src[t];
        if (s == t) continue;
        if (s >= 0) {
            for (int l = j; l < L; l += G) W[(size_t)t * L + l] = W[(size_t)s * L + l];
        } else if (effort_finite(s_e[t])) {
            const double gn = sqrt(E / s_e[t]);
            for (int l = j; l < L; l += G) {
                const C2<T> x = W[(size_t)t * L + l];
                W[(size_t)t * L + l] = c2<T>((T)((double)x.x * gn), (T)((double)x.y * gn));
            }
        }
    }
}

template <typename T>
hipError_t launch_effort(int K, int nV, int L, const EffortArgs& a, hipStream_t s) {
    EffortJobs<T> jobs{};
    jobs.zones = a.zones;
    jobs.emit_hop = a.emit_hop;
    jobs.hop_w = a.hop_w;
    jobs.hop_bins = a.hop_bins;
    for (int z = 0; z < a.zones; ++z) {
        jobs.w[z] = (C2<T>*)a.w[z];
        jobs.limit[z] = a.limit[z];
        jobs.effort[z] = a.effort[z];
        jobs.src[z] = a.src[z];
        jobs.gain[z] = a.gain[z];
    }
    int gsh = 0;
    while (gsh < 6 && (1 << gsh) < L) ++gsh;
    hipLaunchKernelGGL(limit_effort_kernel<T>, dim3(K, 1, a.zones * a.n_hops), dim3(64), 0, s, jobs, nV, L, gsh);
    return hipGetLastError();
}

}  // namespace

hipError_t apv_launch_limit_effort(int c128, int K, int nV, int L, const EffortArgs& a, hipStream_t s, std::string* why) {
    if (K < 1 || nV < 1 || nV > APV_EFFORT_MAX_SLOTS || L < 1 || a.zones < 1 || a.zones > 2 || a.n_hops < 1 ||
        (long long)a.zones * a.n_hops > 65535) {
        if (why) *why = "effort limit: K >= 1, 1 <= nV <= 128, L >= 1, one or two zone programs, zone programs x hops <= 65535";
        return hipErrorInvalidValue;
    }
    const bool emits = a.emit_hop != EFFORT_EMIT_NONE;
    for (int z = 0; z < a.zones; ++z)
        if (!a.w[z] || !a.limit[z] || (emits && (!a.effort[z] || !a.src[z] || !a.gain[z]))) {
            if (why) *why = "effort limit: null filters, limit table or outputs";
            return hipErrorInvalidValue;
        }
    return c128 ? launch_effort<double>(K, nV, L, a, s) : launch_effort<float>(K, nV, L, a, s);
}
