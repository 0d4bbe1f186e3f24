// The per-bin span of the variable-span filter: a mu per bin, a rank cap per bin and the rank that holds a
// contrast floor.  Shared by the four per-bin kernels (kernels_gevd16m.hip, kernels_gevd.hip, kernels_gevd64.hip,
// kernels_gevd128.hip), which keep the same three arrays in LDS at their stage 6: the eigenvalues and the coefficients
// a_i = (u_i^H r) / (lambda_i + mu_k), both indexed by the UNSORTED column, and the descending order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// tables and outputs of one zone program; every pointer may be null (that part is absent)
struct SpanZone {
    const double* mu_eff;     // [K]     mu * profile, formed by the host in double
    const int32_t* cap;       // [K]     rank cap, 1..L
    int32_t* rank;            // [K]     min(top rank of the list, s_k); 0 in a bin of status 1
    double* contrast;         // [K][L]  c_v, written only with a floor
};

struct SpanParams {
    int on;                   // 0: the launch has no span; nothing below is read (one uniform branch)
    double phi;               // contrast floor 10^(dB / 10); 0: none
    SpanZone z[2];            // [0]: the launch's first zone program (w, lam, status), [1]: its second (w1, lam1, status1)
    // a launch of several hops (GevdParams::n_hops > 1) writes the outputs of its last hop only: hop stride 0, one writer
    int last_hop;
};

#if defined(__HIPCC__)
// mu of bin k of the launch's first (z1 = false) or second zone program: the table's entry, or the launch's common mu.  (Selects
// between constant members, here and below, as the kernels pick w / w1: the argument block stays in scalar registers.)
// SPAN = false (here and below): the kernel instantiation of launches without a span, which holds none of this code.
template <bool SPAN, typename T>
__device__ __forceinline__ T span_mu(const SpanParams& sp, bool z1, int k, double mu) {
    if constexpr (SPAN) {
        if (sp.on) {
            const double* const t = z1 ? sp.z[1].mu_eff : sp.z[0].mu_eff;
            if (t != nullptr) return (T)t[k];
        }
    }
    return (T)mu;
}

// s_k = min(cap_k, f_k) of bin k: the largest rank its output slots may reach (n without a span).  Every thread of the workgroup
// calls it behind the barrier that publishes lam / coef / order and gets the same value: each walks the n sorted terms itself
// (LDS broadcast reads), so no further barrier is needed.  Thread v < n writes c_v, thread 0 the rank.
//   num_v = sum_{i <= v} lambda_i |a_i|^2,  den_v = sum_{i <= v} |a_i|^2,  c_v = num_v / den_v (0 where den_v = 0)
//   f_k = number of leading v with num_v >= phi den_v (at least 1)
// ok: the bin was solved (status != 1); emit: this launch (hop) writes the outputs; top: the last rank of the list.
template <bool SPAN, typename T, typename C>
__device__ __forceinline__ int span_limit(const SpanParams& sp, bool z1, int k, int n, int top, bool ok, bool emit, const T* lam,
                                          const C* coef, const int* order, int tid) {
    if constexpr (!SPAN) return n;
    if (!sp.on) return n;
    const int32_t* const pcap = z1 ? sp.z[1].cap : sp.z[0].cap;
    int32_t* const prank = z1 ? sp.z[1].rank : sp.z[0].rank;
    double* const pc = (emit && sp.phi > 0.0) ? (z1 ? sp.z[1].contrast : sp.z[0].contrast) : nullptr;
    int lim = n;
    if (ok && sp.phi > 0.0) {
        const T phi = (T)sp.phi;
        T num = 0, den = 0;
        int f = 0;
        bool run = true;
        // (rolled: n dependent steps, nothing to gain from unrolling at a compile-time order)
#pragma nounroll
        for (int v = 0; v < n; ++v) {
            const int c = order[v];
            const C a = coef[c];
            const T e = a.x * a.x + a.y * a.y;
            den += e;
            num += lam[c] * e;
            run = run && (num >= phi * den);
            f += run ? 1 : 0;
            if (pc != nullptr && tid == v) pc[(size_t)k * n + v] = den > (T)0 ? (double)(num / den) : 0.0;
        }
        lim = f > 1 ? f : 1;
    } else if (pc != nullptr && tid < n) {
        pc[(size_t)k * n + tid] = 0.0;
    }
    if (pcap != nullptr) {
        const int cap = pcap[k];
        lim = cap < lim ? cap : lim;
    }
    if (emit && prank != nullptr && tid == 0) prank[k] = ok ? (top < lim ? top : lim) : 0;
    return lim;
}
#endif
