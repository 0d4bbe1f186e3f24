// Filter-length constraint of the subband stream (apv_stream_set_filter_taps): every per-bin filter W[:, v, l] of a hop is
// projected onto the spectra of J-tap impulse responses,
//
//   g = irfft(W[:, v, l], N);  g[J:] = 0;  W'[:, v, l] = rfft(g, N)           the reference's w_A / w_B are J-tap FIR filters,
//                                                                            apvast.py:406-422; here per (rank, loudspeaker)
//
// the constraint step of frequency-domain adaptive filters.  The filters are stored bin-major, [K][nV][L]: one channel's bins
// lie nV L elements apart, one bin's L loudspeakers side by side.  A workgroup therefore takes TL neighbouring loudspeakers of one
// (zone program, rank): blockDim = (STFT_TPB, TL), row y of the workgroup transforms loudspeaker l0 + y in an LDS slice of its
// own with the device code of the STFT kernels (stft_fft.h reads threadIdx.x only, and its barriers are met by every row: the
// rows run the same plan).  Global loads and stores go through a flat index whose fastest digit is the loudspeaker, so that
// neighbouring lanes touch the TL contiguous elements of a bin -- one 64-byte line of complex128 at TL = 4.  The LDS slices are
// the transpose buffer: bins 1 .. N/2 - 1 sit in their slots, the two real bins 0 and N/2 share slot 0.
//
// TL is the largest of 4, 2, 1 whose slices fit 64 KB (a float64 Bluestein transform at M = 4096 fills that alone).
//
// The filters of several hops in one launch (apv_launch_constrain_filters_hops, the chunked whole-signal path): blockIdx.z = hop x
// zone program, hop i's filters hop_w elements behind those of hop i - 1 and its taps hop_taps elements behind.  Plan, TL, LDS
// per workgroup and the arithmetic of a channel are those of the launch of one hop.
#include "apv_internal.h"
#include "stft_fft.h"

namespace {

constexpr int CF_MAX_TL = 4;          // loudspeakers per workgroup: 4 x STFT_TPB = 1024 threads
constexpr size_t CF_LDS_BUDGET = 64 * 1024;

template <typename T>
struct ConstrainJobs {
    C2<T>* w[2];          // [K][nV][L] per zone program of the launch, projected in place
    T* taps[2];           // [nV][J][L]: g[:J] of every channel (may be null)
    int zones;            // blockIdx.z = hop * zones + zone program
    size_t hop_w;         // elements from one hop's filters / taps to the next hop's (a launch of one hop multiplies them by its
    size_t hop_taps;      // hop index, 0)
};

template <typename T, int MI, bool BS>
__global__ void __launch_bounds__(STFT_TPB * CF_MAX_TL) constrain_filters_kernel(FftPlan plan, ConstrainJobs<T> jobs, int nV, int L,
                                                                                int J, const C2<T>* __restrict__ tw) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int Nh = plan.Nh, tid = threadIdx.x, ty = threadIdx.y, TL = blockDim.y;
    const int tl_sh = __ffs(TL) - 1;                                       // TL is a power of two
    const size_t slice = (size_t)(plan.inplace ? 1 : 2) * plan.buf;        // complex elements of one row's LDS
    C2<T>* const base = reinterpret_cast<C2<T>*>(smem_raw);
    C2<T>* const za = base + ty * slice;
    C2<T>* const zb = za + plan.buf;
    const int v = blockIdx.y, hop = blockIdx.z / jobs.zones, zone = blockIdx.z - hop * jobs.zones, l0 = blockIdx.x * TL;
    const size_t sk = (size_t)nV * L;                                      // elements from bin to bin
    C2<T>* __restrict__ W = jobs.w[zone] + (size_t)hop * jobs.hop_w + (size_t)v * L + l0;
    const int flat = ty * STFT_TPB + tid, nthr = STFT_TPB * TL;

    // bins in, loudspeaker fastest: slot k of row lt takes bin k, slot 0 the real parts of bins 0 and N/2 (irfft drops their
    // imaginary parts); rows beyond the last loudspeaker transform zeros
    for (int e = flat; e < (Nh + 1) * TL; e += nthr) {
        const int k = e >> tl_sh, lt = e & (TL - 1);
        const C2<T> x = (l0 + lt < L) ? W[(size_t)k * sk + lt] : c2<T>((T)0, (T)0);
        C2<T>* s = base + lt * slice;
        if (k == 0) s[0].x = x.x;
        else if (k == Nh) s[0].y = x.x;
        else s[k] = x;
    }
    __syncthreads();
    // Z[k] = E[k] + i O[k] packed for the half-length inverse transform conj(FFT(conj(Z))) / Nh, as istft_ola_kernel packs it; in
    // place, so a thread takes slots k and Nh - k together
    auto pack = [&](C2<T> a, C2<T> bq, C2<T> wk) {
        const C2<T> b = c2<T>(bq.x, -bq.y);
        const C2<T> e = c2<T>((T)0.5 * (a.x + b.x), (T)0.5 * (a.y + b.y));
        const C2<T> dm = c2<T>((T)0.5 * (a.x - b.x), (T)0.5 * (a.y - b.y));
        const C2<T> o = cmul(dm, c2<T>(wk.x, -wk.y));
        return c2<T>(e.x - o.y, -(e.y + o.x));
    };
    for (int k = tid; 2 * k <= Nh; k += STFT_TPB) {
        if (k == 0) {
            const C2<T> s0 = za[0];
            za[0] = pack(c2<T>(s0.x, (T)0), c2<T>(s0.y, (T)0), tw[0]);
        } else {
            const int k2 = Nh - k;
            const C2<T> a = za[k], bq = za[k2];
            za[k] = pack(a, bq, tw[k]);
            if (k2 != k) za[k2] = pack(bq, a, tw[k2]);
        }
    }
    __syncthreads();
    C2<T>* z = fft_forward<T, MI, BS>(plan, za, zb, tw);
    // g[2n] = Re z[n] / Nh, g[2n + 1] = -Im z[n] / Nh; taps J and later go, and the pair is the input of the forward transform
    const T scale = (T)1 / (T)Nh;
    for (int n = tid; n < Nh; n += STFT_TPB) {
        const C2<T> q = z[n];
        z[n] = c2<T>(2 * n < J ? q.x * scale : (T)0, 2 * n + 1 < J ? -q.y * scale : (T)0);
    }
    __syncthreads();
    if (jobs.taps[zone] != nullptr) {
        T* __restrict__ tp = jobs.taps[zone] + (size_t)hop * jobs.hop_taps + (size_t)v * J * L + l0;
        const size_t zoff = z - za;                                        // the same for every row
        for (int e = flat; e < J * TL; e += nthr) {
            const int j = e >> tl_sh, lt = e & (TL - 1);
            if (l0 + lt < L) tp[(size_t)j * L + lt] = reinterpret_cast<const T*>(base + lt * slice + zoff)[j];
        }
        __syncthreads();                                                   // the transform below overwrites the taps
    }
    z = fft_forward<T, MI, BS>(plan, z, z == za ? zb : za, tw);
    // even/odd split X[k] = E[k] + e^{-2 pi i k / N} O[k] as rfft_from_lds forms it; in place again, bins 0 and N/2 (both real) to slot 0
    auto split = [&](C2<T> a, C2<T> bq, C2<T> wk) {
        const C2<T> b = c2<T>(bq.x, -bq.y);
        const C2<T> e = c2<T>((T)0.5 * (a.x + b.x), (T)0.5 * (a.y + b.y));
        const C2<T> dm = c2<T>((T)0.5 * (a.x - b.x), (T)0.5 * (a.y - b.y));
        const C2<T> ow = cmul(c2<T>(dm.y, -dm.x), wk);
        return c2<T>(e.x + ow.x, e.y + ow.y);
    };
    for (int k = tid; 2 * k <= Nh; k += STFT_TPB) {
        if (k == 0) {
            const C2<T> z0 = z[0];
            z[0] = c2<T>(z0.x + z0.y, z0.x - z0.y);
        } else {
            const int k2 = Nh - k;
            const C2<T> a = z[k], bq = z[k2];
            z[k] = split(a, bq, tw[k]);
            if (k2 != k) z[k2] = split(bq, a, tw[k2]);
        }
    }
    __syncthreads();
    const size_t zoff = z - za;
    for (int e = flat; e < (Nh + 1) * TL; e += nthr) {
        const int k = e >> tl_sh, lt = e & (TL - 1);
        if (l0 + lt >= L) continue;
        const C2<T>* s = base + lt * slice + zoff;
        W[(size_t)k * sk + lt] = k == 0 ? c2<T>(s[0].x, (T)0) : k == Nh ? c2<T>(s[0].y, (T)0) : s[k];
    }
}

template <typename T>
hipError_t launch_constrain(const FftPlan& plan, int J, int nV, int L, int zones, void* const* w, void* const* taps, int n_hops,
                            size_t hop_w, size_t hop_taps, hipStream_t s) {
    const void* tw = nullptr;
    hipError_t e = apv_stft_tables(sizeof(T) == 8, plan.N, &tw);
    if (e != hipSuccess) return e;
    const size_t lds = apv_stft_plan_lds(plan, sizeof(T) == 8);
    int TL = CF_MAX_TL;
    while (TL > 1 && (TL * lds > CF_LDS_BUDGET || TL / 2 >= L)) TL /= 2;
    ConstrainJobs<T> jobs{};
    jobs.zones = zones;
    jobs.hop_w = hop_w;
    jobs.hop_taps = hop_taps;
    for (int z = 0; z < zones; ++z) {
        jobs.w[z] = (C2<T>*)w[z];
        jobs.taps[z] = taps ? (T*)taps[z] : nullptr;
    }
    const auto kern = plan.bluestein ? (plan.max_it == 1 ? constrain_filters_kernel<T, 1, true> : constrain_filters_kernel<T, INPLACE_MAX_IT, true>)
                                     : (plan.max_it == 1 ? constrain_filters_kernel<T, 1, false> : constrain_filters_kernel<T, INPLACE_MAX_IT, false>);
    hipLaunchKernelGGL(kern, dim3((L + TL - 1) / TL, nV, zones * n_hops), dim3(STFT_TPB, TL), TL * lds, s, plan, jobs, nV, L, J, (const C2<T>*)tw);
    return hipGetLastError();
}

}  // namespace

// can the projection run at block size N with filters stored in double (c128) or float?  One transform has to fit 64 KB of LDS.
bool apv_constrain_size_ok(int c128, int N, std::string* why) {
    FftPlan plan;
    if (!apv_stft_make_plan(N, &plan, why)) return false;
    if (apv_stft_plan_lds(plan, c128) > CF_LDS_BUDGET) {
        if (why) *why = "filter constraint: one transform of this block size in the filters' precision does not fit 64 KB of LDS";
        return false;
    }
    return true;
}

// w[z] [N/2 + 1][nV][L] complex (c128: double, else float) of `zones` zone programs projected in place onto J-tap responses, the
// taps g[:J] to taps[z] [nV][J][L] real of the same precision (taps or taps[z] may be null); 1 <= J <= N.  n_hops > 1: the same for
// the n_hops filter sets w[z] + i hop_w (elements), the taps of set i to taps[z] + i hop_taps, in one launch (grid.z = hop x zone
// program); every (hop, zone program, rank, loudspeaker tile) is the workgroup the launch of that hop alone runs
hipError_t apv_launch_constrain_filters_hops(int c128, int N, int J, int nV, int L, int zones, void* const* w, void* const* taps,
                                             int n_hops, size_t hop_w, size_t hop_taps, hipStream_t s, std::string* why) {
    FftPlan plan;
    if (!apv_constrain_size_ok(c128, N, why) || !apv_stft_make_plan(N, &plan, why)) return hipErrorInvalidValue;
    if (J < 1 || J > N || nV < 1 || nV > 65535 || L < 1 || zones < 1 || zones > 2 || n_hops < 1 || zones * n_hops > 65535) {
        if (why) *why = "filter constraint: 1 <= J <= N, 1 <= nV <= 65535, L >= 1, one or two zone programs, zone programs x hops <= 65535";
        return hipErrorInvalidValue;
    }
    return c128 ? launch_constrain<double>(plan, J, nV, L, zones, w, taps, n_hops, hop_w, hop_taps, s)
                : launch_constrain<float>(plan, J, nV, L, zones, w, taps, n_hops, hop_w, hop_taps, s);
}

hipError_t apv_launch_constrain_filters(int c128, int N, int J, int nV, int L, int zones, void* const* w, void* const* taps,
                                        hipStream_t s, std::string* why) {
    return apv_launch_constrain_filters_hops(c128, N, J, nV, L, zones, w, taps, 1, 0, 0, s, why);
}
