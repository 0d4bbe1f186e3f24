// The transform device code shared by the translation units that run FFTs in LDS (kernels_stft.hip: K2-K4 and the fast
// convolution; kernels_constrain.hip: the filter-length projection): plan, complex helpers, the mixed-radix 4/2/3/5/7 Stockham
// stages, their one-buffer form and the Bluestein (chirp-z) transform.  Plans and tables are made by kernels_stft.hip
// (apv_stft_make_plan, apv_stft_tables): one table set per (device, N, dtype) whoever asks.
#pragma once
#include <hip/hip_runtime.h>
#include <string>

constexpr int STFT_TPB = 256;
constexpr int STFT_MAX_N = 8192;
constexpr int STFT_MAX_BLUESTEIN_N = 4096;    // M <= 4096: one in-place buffer (64 KB of double), M/4 <= INPLACE_MAX_IT * STFT_TPB
constexpr int MAX_STAGES = 14;

struct FftPlan {
    int N;                 // real length
    int Nh;                // complex length N/2
    int nstages;
    int radix[MAX_STAGES];
    int inplace;           // every stage is radix 4 or 2 and short enough for stockham_stage_inplace: ONE LDS buffer of Nh
    int bluestein;         // N/2 is not 7-smooth: chirp-z transform; radix[] / nstages are then the stages of the M-point transforms
    int M;                 // Bluestein convolution length, the power of two >= 2 Nh - 1 (0 for a 7-smooth plan)
    int buf;               // complex elements of one LDS buffer: Nh, or M for a Bluestein plan (the second buffer starts there)
    int max_it;            // butterflies per thread of the widest in-place stage (kernels are instantiated for 1 and for INPLACE_MAX_IT)
    int debug;             // timing aids of the analysis transforms (APV_STFT_DEBUG; results are wrong): 1 no spectrum stores, 2 no sample loads, 4 no stages
};
constexpr int INPLACE_MAX_IT = 4;      // butterflies per thread and stage the in-place form holds in registers

namespace {

// 16-byte alignment for the double-precision pair: the compiler then moves it as ONE ds_read_b128 / ds_write_b128 / dwordx4
// (4 LDS cycles per wave-instruction where the two ds_read2_b64 halves of an 8-byte-aligned pair cost 16, and sixteen lanes a
// group at a 16-byte stride are a 2-way bank conflict on top: SQ_LDS_BANK_CONFLICT was 61 % of the LDS-active cycles of every
// transform kernel, profiles/r03/analysis_counters.md)
template <typename T> struct alignas(2 * sizeof(T)) C2 { T x, y; };
template <typename T> __device__ __forceinline__ C2<T> c2(T a, T b) { C2<T> r; r.x = a; r.y = b; return r; }
template <typename T> __device__ __forceinline__ C2<T> cadd(C2<T> a, C2<T> b) { return c2<T>(a.x + b.x, a.y + b.y); }
template <typename T> __device__ __forceinline__ C2<T> csub(C2<T> a, C2<T> b) { return c2<T>(a.x - b.x, a.y - b.y); }
template <typename T> __device__ __forceinline__ C2<T> cmul(C2<T> a, C2<T> b) {
    return c2<T>(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// ---- Stockham stages ---------------------------------------------------------------------------
// One stage of radix R: sub-transforms of length Ns become length Ns*R.  tw is the N-entry root table;
// the roots of the Nh-point transform are its even entries.
template <typename T, int R>
__device__ __forceinline__ void stockham_stage(const C2<T>* __restrict__ src, C2<T>* __restrict__ dst, int Nh, int Ns,
                                               const C2<T>* __restrict__ tw, int N) {
    const int m = Nh / R;
    const int tstep = 2 * (Nh / (Ns * R));            // tw index step for exp(-2 pi i k / (Ns R))
    // j = q Ns + k: a shift and a mask while the sub-transform length is a power of two (every stage of a power-of-two block,
    // the leading stages of a mixed-radix one); integer division is ~25 instructions on this machine, more than the butterfly
    const bool pow2 = (Ns & (Ns - 1)) == 0;
    const int sh = __ffs(Ns) - 1;
    for (int j = threadIdx.x; j < m; j += STFT_TPB) {
        const int q = pow2 ? (j >> sh) : (j / Ns);
        const int k = j - q * Ns;
        C2<T> u[R];
#pragma unroll
        for (int t = 0; t < R; ++t) u[t] = src[j + t * m];
        // twiddles w^t, w = exp(-2 pi i k / (Ns R)): none in the first stage (k = 0); radix 4 fetches w alone and squares and
        // cubes it (a table read is an L2 round trip on the critical path of the stage, a complex product is four FMAs)
        if (Ns > 1) {
            if constexpr (R == 4) {
                const C2<T> w1 = tw[k * tstep], w2 = cmul(w1, w1), w3 = cmul(w2, w1);
                u[1] = cmul(u[1], w1);
                u[2] = cmul(u[2], w2);
                u[3] = cmul(u[3], w3);
            } else {
#pragma unroll
                for (int t = 1; t < R; ++t) u[t] = cmul(u[t], tw[t * k * tstep]);   // t k tstep <= (R-1)(Ns-1) N / (Ns R) < N: no wrap
            }
        }
        C2<T> v[R];
        if constexpr (R == 2) {
            v[0] = cadd(u[0], u[1]);
            v[1] = csub(u[0], u[1]);
        } else if constexpr (R == 4) {
            const C2<T> a = cadd(u[0], u[2]), b = csub(u[0], u[2]), c = cadd(u[1], u[3]), d = csub(u[1], u[3]);
            v[0] = cadd(a, c);
            v[2] = csub(a, c);
            v[1] = c2<T>(b.x + d.y, b.y - d.x);       // b - i d
            v[3] = c2<T>(b.x - d.y, b.y + d.x);       // b + i d
        } else {
            // direct DFT of prime length R with the roots w_R^q = tw[q N / R]
            const int rstep = N / R;
#pragma unroll
            for (int o = 0; o < R; ++o) {
                C2<T> acc = u[0];
#pragma unroll
                for (int t = 1; t < R; ++t) acc = cadd(acc, cmul(u[t], tw[((o * t) % R) * rstep]));
                v[o] = acc;
            }
        }
        const int base = q * Ns * R + k;
#pragma unroll
        for (int t = 0; t < R; ++t) dst[base + t * Ns] = v[t];
    }
}

// The same stage on ONE buffer: every thread reads the inputs of all its butterflies, the workgroup meets, the outputs
// go back to the same array.  Two barriers per stage instead of one, half the LDS: at 16 KB instead of 32 KB per
// 2048-point double-precision transform eight workgroups fit a CU instead of five -- and five instead of two beside
// the streaming pipeline's joint diagonalisation, which holds 80 KB of every CU while the next hop's transforms run.
template <typename T, int R, int MI = INPLACE_MAX_IT>
__device__ __forceinline__ void stockham_stage_inplace(C2<T>* __restrict__ buf, int Nh, int Ns, const C2<T>* __restrict__ tw) {
    // MI: butterflies per thread held in registers across the barrier.  The array below is sized by it, whatever the plan needs at run
    // time: with MI = 4 the float64 transforms carried 64 VGPRs of it (101 in all: five workgroups per CU) although a 2048-point
    // block needs ONE butterfly per thread and stage; the hot kernels are therefore instantiated for MI = 1 as well (plan.max_it).
    static_assert(R == 2 || R == 4, "in-place stages are radix 2 or 4");
    const int m = Nh / R;
    const int tstep = 2 * (Nh / (Ns * R));
    const int sh = __ffs(Ns) - 1;                      // Ns is a power of two here
    C2<T> v[MI][R];
#pragma unroll
    for (int it = 0; it < MI; ++it) {
        const int j = threadIdx.x + it * STFT_TPB;
        if (j >= m) break;
        const int k = j & (Ns - 1);
        C2<T> u[R];
#pragma unroll
        for (int t = 0; t < R; ++t) u[t] = buf[j + t * m];
        if (Ns > 1) {
            const C2<T> w1 = tw[k * tstep];
            u[1] = cmul(u[1], w1);
            if constexpr (R == 4) {
                const C2<T> w2 = cmul(w1, w1), w3 = cmul(w2, w1);
                u[2] = cmul(u[2], w2);
                u[3] = cmul(u[3], w3);
            }
        }
        if constexpr (R == 2) {
            v[it][0] = cadd(u[0], u[1]);
            v[it][1] = csub(u[0], u[1]);
        } else {
            const C2<T> a = cadd(u[0], u[2]), b = csub(u[0], u[2]), c = cadd(u[1], u[3]), d = csub(u[1], u[3]);
            v[it][0] = cadd(a, c);
            v[it][2] = csub(a, c);
            v[it][1] = c2<T>(b.x + d.y, b.y - d.x);
            v[it][3] = c2<T>(b.x - d.y, b.y + d.x);
        }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MI; ++it) {
        const int j = threadIdx.x + it * STFT_TPB;
        if (j >= m) break;
        const int q = j >> sh, k = j & (Ns - 1);
        const int base = q * Ns * R + k;
#pragma unroll
        for (int t = 0; t < R; ++t) buf[base + t * Ns] = v[it][t];
    }
    __syncthreads();
}

// Bluestein (chirp-z) form of the Nh-point DFT for an Nh with a prime factor above 7.  With c[n] = exp(-i pi n^2 / Nh) and
// n k = (n^2 + k^2 - (k - n)^2) / 2,  X[k] = c[k] sum_n (x[n] c[n]) conj(c[k - n]):  a circular convolution of length M >= 2 Nh - 1,
// i.e. a product of M-point spectra, the kernel's (B / M) from the tables.  The input sits in a[0, Nh) and the workgroup has met; a
// holds M elements.  The inverse transform is conj(FFT(conj(.))), its 1/M folded into B; the Nh results end in a[0, Nh).
template <typename T, int MI>
__device__ __forceinline__ void fft_bluestein(const FftPlan& plan, C2<T>* a, const C2<T>* __restrict__ tw) {
    const int Nh = plan.Nh, M = plan.M, tid = threadIdx.x;
    const C2<T>* __restrict__ twm = tw + plan.N;          // exp(-i pi j / M): the M-point stages read it like tw for Nh
    const C2<T>* __restrict__ chirp = twm + M;
    const C2<T>* __restrict__ bh = chirp + Nh;
    for (int n = tid; n < M; n += STFT_TPB) a[n] = n < Nh ? cmul(a[n], chirp[n]) : c2<T>((T)0, (T)0);
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        int Ns = 1;
        for (int s = 0; s < plan.nstages; ++s) {          // every stage ends on a barrier
            if (plan.radix[s] == 4) stockham_stage_inplace<T, 4, MI>(a, M, Ns, twm);
            else stockham_stage_inplace<T, 2, MI>(a, M, Ns, twm);
            Ns *= plan.radix[s];
        }
        if (pass == 0)
            for (int n = tid; n < M; n += STFT_TPB) {
                const C2<T> y = cmul(a[n], bh[n]);
                a[n] = c2<T>(y.x, -y.y);
            }
        else
            for (int n = tid; n < Nh; n += STFT_TPB) {
                const C2<T> z = a[n];
                a[n] = cmul(c2<T>(z.x, -z.y), chirp[n]);
            }
        __syncthreads();
    }
}

// forward complex FFT of length plan.Nh on natural-order data in `a`; returns the buffer holding the result (`b` is not
// touched, and need not exist, when plan.inplace is set).  BS: the kernel is instantiated for Bluestein plans (fft_bluestein);
// the 7-smooth instantiations carry none of its code
template <typename T, int MI = INPLACE_MAX_IT, bool BS = false>
__device__ __forceinline__ C2<T>* fft_forward(const FftPlan& plan, C2<T>* a, C2<T>* b, const C2<T>* __restrict__ tw) {
    if constexpr (BS) {
        fft_bluestein<T, MI>(plan, a, tw);
        return a;
    }
    if (plan.inplace) {
        int Ns = 1;
        for (int s = 0; s < plan.nstages; ++s) {
            if (plan.radix[s] == 4) stockham_stage_inplace<T, 4, MI>(a, plan.Nh, Ns, tw);
            else stockham_stage_inplace<T, 2, MI>(a, plan.Nh, Ns, tw);
            Ns *= plan.radix[s];
        }
        return a;
    }
    int Ns = 1;
    C2<T>* src = a;
    C2<T>* dst = b;
    for (int s = 0; s < plan.nstages; ++s) {
        const int R = plan.radix[s];
        switch (R) {
            case 4: stockham_stage<T, 4>(src, dst, plan.Nh, Ns, tw, plan.N); break;
            case 2: stockham_stage<T, 2>(src, dst, plan.Nh, Ns, tw, plan.N); break;
            case 3: stockham_stage<T, 3>(src, dst, plan.Nh, Ns, tw, plan.N); break;
            case 5: stockham_stage<T, 5>(src, dst, plan.Nh, Ns, tw, plan.N); break;
            default: stockham_stage<T, 7>(src, dst, plan.Nh, Ns, tw, plan.N); break;
        }
        __syncthreads();
        Ns *= R;
        C2<T>* t = src; src = dst; dst = t;
    }
    return src;
}

}  // namespace

// kernels_stft.hip: the plan of a block size (false and *why when N is refused), LDS bytes of one transform of it in float (f64 = 0) or
// double, and the root / chirp tables of (current device, N, dtype), built at the first call (C2<float> or C2<double> entries)
bool apv_stft_make_plan(int N, FftPlan* plan, std::string* why);
size_t apv_stft_plan_lds(const FftPlan& plan, int f64);
hipError_t apv_stft_tables(int f64, int N, const void** tw);
