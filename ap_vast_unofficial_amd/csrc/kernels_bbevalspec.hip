// Per-bin evaluation spectra of the broadband stream (apv_bb_set_evaluation_spectra): behind the evaluation stage of a launch over
// n hops (kernels_bbeval.hip), whose pressures p [sets][n H][Mv] are consecutive in time, every hop's frame is windowed, transformed
// and |P|^2 accumulated per bin -- the definition of kernels_evalspec.hip, for n hops at once.  With f_t[s][i, m] =
// p[s][(t + 1) H - N + i, m] the frame after hop t (zero before sample 0), w the stream's sine window and P_t[s][k, m] =
// rfft(w f_t[s][:, m])[k], k < K = N/2 + 1, unnormalised:
//
//   bright[z, v, m, k] += |P_bright|^2        dark[z, v, m, k] += |P_dark|^2
//   error [z, v, m, k] += |P_target - P_bright|^2        target[z, m, k] += |P_target|^2
//
// Three launches per (sub-)launch of c hops, everything float64:
//
// 1. bbspec_line_kernel.  Per pressure set and microphone a LINE of N - H + c H consecutive samples, channel-major
// [sets Mv][N - H + c H]: the newest N - H samples from before the launch (the last N - H of the previous line, whatever its
// length was), then the launch's c H pressures, transposed.  Frame i of a channel starts i H samples into its line: no ring, no
// wrap, nothing special where H does not divide N.  The tail may be longer than the launch, and workgroups read what others
// write, so the lines alternate between two buffers: old line in, new line out.  A workgroup moves a tile of 16 samples x 16
// microphones; the pressures go through LDS (rows padded to 17), read in runs of 16 microphones and written in runs of 16
// samples (128 bytes either side); the tail is read as it is written.  H = N: no tail, the line is the launch.
//
// 2. The stream's own analysis launch (apv_launch_stft_analysis_chunk, float64) on the line buffer: one channel set of sets Mv
// channels, rows N - H + c H long, frames H apart, into the bin-major scratch [c][K][sets Mv] complex128.  Bluestein sizes
// included; the same launch for c = 1.
//
// 3. bbspec_energy_kernel.  One thread per element of the totals [Z][3 E + 1][K][Mv], microphones fastest as in the scratch: it
// adds the c hops in hop order, total = total + |P|^2, the squared magnitude written once for every hop.  No atomics; one owner per
// element, so the bits depend on the data and the hop order alone -- not on c, not on a hop's place in a launch, not on the grid.
//
// The scratch has a fixed byte budget (APV_BBSPEC_SCRATCH_BYTES, at least one hop): a group of hops runs as consecutive
// sub-launches of as many hops as fit, which by the property of 3 changes no bit.
//
// With the detectability switch (apv_bb_set_evaluation_detectability) the three hop-batched launches of kernels_evaldetect.hip
// follow 3 inside every sub-launch, on the scratch the next sub-launch overwrites; their bits do not depend on c either.
//
// Bounds: every access of 1 and 3 is predicated; H, Mv, N and c need not be multiples of anything.  Nothing is read past
// [sets][n H][Mv] pressures, the old line's [sets Mv][old length] and [c][K][sets Mv] spectra; nothing is written past
// [sets Mv][N - H + c H] line samples and the totals.
#include "apv_internal.h"

#include <algorithm>

namespace {

constexpr int BS_T = 16;                       // tile edge: 16 samples x 16 microphones, one element per thread

// p: the launch's first pressure row of set 0, the sets p_set elements apart; old_len >= N - H = tail
__global__ void __launch_bounds__(256) bbspec_line_kernel(const double* __restrict__ p, size_t p_set, const double* __restrict__ old_line,
                                                          long long old_len, double* __restrict__ new_line, long long len, int tail,
                                                          int Mv) {
    __shared__ double tile[BS_T][BS_T + 1];
    const int set = blockIdx.z, m0 = blockIdx.y * BS_T;
    const long long j0 = (long long)blockIdx.x * BS_T;
    const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
    // in: neighbouring threads along the microphones
    if (j0 + a >= tail && j0 + a < len && m0 + b < Mv) tile[a][b] = p[(size_t)set * p_set + (size_t)(j0 + a - tail) * Mv + m0 + b];
    __syncthreads();
    // out: neighbouring threads along the samples
    const int m = m0 + a;
    const long long j = j0 + b;
    if (m < Mv && j < len) {
        const size_t ch = (size_t)set * Mv + m;
        new_line[ch * len + j] = j < tail ? old_line[ch * old_len + (old_len - tail) + j] : tile[b][a];
    }
}

__device__ __forceinline__ double sqmag(double x, double y) { return fma(x, x, y * y); }

__global__ void __launch_bounds__(256) bbspec_energy_kernel(const double2* __restrict__ spec, double* __restrict__ totals, int Z, int E,
                                                            int K, int Mv, int n) {
    const int per_z = 3 * E + 1;
    const size_t items = (size_t)Z * per_z * K * Mv, it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int m = (int)(it % Mv), k = (int)((it / Mv) % K);
    const int q = (int)((it / ((size_t)Mv * K)) % per_z), z = (int)(it / ((size_t)Mv * K * per_z));
    const size_t row = (size_t)Z * (2 * E + 1) * Mv, hop = (size_t)K * row;       // channels of one bin, elements of one hop
    const double2* __restrict__ sz = spec + (size_t)k * row + (size_t)z * (2 * E + 1) * Mv + m;
    const bool diff = q >= 2 * E && q < 3 * E;
    // the set squared, or with diff subtracted from the target first
    const double2* __restrict__ sa = sz + (size_t)(q < 2 * E ? q : (diff ? q - 2 * E : 2 * E)) * Mv;
    const double2* __restrict__ st = sz + (size_t)2 * E * Mv;
    double tot = totals[it];
    if (diff) {
        for (int i = 0; i < n; ++i) {
            const double2 t = st[(size_t)i * hop], br = sa[(size_t)i * hop];
            tot = tot + sqmag(t.x - br.x, t.y - br.y);
        }
    } else {
        for (int i = 0; i < n; ++i) {
            const double2 v = sa[(size_t)i * hop];
            tot = tot + sqmag(v.x, v.y);
        }
    }
    totals[it] = tot;
}

}  // namespace

bool apv_bbspec_size_ok(int N, int H, int Z, int E, int Mv, std::string* why) {
    if (!apv_eval_spectra_size_ok(N, H, Z, E, Mv, why)) return false;
    if (((size_t)Z * (3 * (size_t)E + 1) * (N / 2 + 1) * Mv + 255) / 256 > 0x7fffffffull) {
        if (why) *why = "evaluation spectra: the totals [Z][3 E + 1][K][Mv] must stay below 2^39 elements";
        return false;
    }
    return true;
}

int apv_bbspec_hops_fit(int N, int Z, int E, int Mv) {
    const size_t hop = sizeof(double) * 2 * ((size_t)N / 2 + 1) * Z * (2 * (size_t)E + 1) * Mv;
    return (int)std::min<size_t>(std::max<size_t>(APV_BBSPEC_SCRATCH_BYTES / hop, 1), 65535);
}

// the detectability of the c hops whose spectra stand at `spec`, hops i0 .. i0 + c - 1 of the call
static hipError_t bbspec_detect(const BbSpecDetectArgs& d, const void* spec, int i0, int c, int N, int Z, int E, int Mv, hipStream_t s,
                                std::string* why) {
    EvalDetectHopsArgs a{};
    a.spec = spec; a.G2T = d.G2T; a.quiet = d.quiet; a.curves = d.curves; a.part = d.part; a.rec = d.rec; a.totals = d.totals;
    a.slot0 = d.slot0 + i0; a.n = c; a.N = N; a.Z = Z; a.E = E; a.Mv = Mv; a.C = d.C;
    a.Cs = d.Cs; a.Ca = d.Ca; a.Leff = d.Leff;
    return apv_launch_eval_detect_hops(a, s, why);
}

hipError_t apv_launch_bbspec_detect_hops(const BbSpecDetectArgs& d, const void* spec, int n, int per_launch, int N, int Z, int E, int Mv,
                                         hipStream_t s, std::string* why) {
    if (!spec || n < 1 || per_launch < 1 || per_launch > 65535) {
        if (why) *why = "evaluation detectability: null spectra, no hops, or 0 hops per launch";
        return hipErrorInvalidValue;
    }
    const size_t hop = sizeof(double) * 2 * ((size_t)N / 2 + 1) * Z * (2 * (size_t)E + 1) * Mv;
    for (int i0 = 0; i0 < n; i0 += per_launch) {
        const hipError_t e = bbspec_detect(d, static_cast<const char*>(spec) + (size_t)i0 * hop, i0, std::min(per_launch, n - i0), N, Z, E,
                                           Mv, s, why);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t apv_launch_bbspec_hops(BbSpecArgs* a, hipStream_t s, std::string* why) {
    if (!apv_bbspec_size_ok(a->N, a->H, a->Z, a->E, a->Mv, why)) return hipErrorInvalidValue;
    const int tail = a->N - a->H;
    if (!a->p || !a->line[0] || !a->line[1] || !a->spec || !a->totals || (a->cur != 0 && a->cur != 1) || a->n < 1 ||
        a->per_launch < 1 || a->per_launch > 65535 || a->len < tail || (long long)a->n * a->H > 0x7fffffffll) {
        if (why) *why = "evaluation spectra: null device pointer, no hops, or a line shorter than N - H";
        return hipErrorInvalidValue;
    }
    const int sets = a->Z * (2 * a->E + 1), K = a->N / 2 + 1;
    const size_t items = (size_t)a->Z * (3 * a->E + 1) * K * a->Mv;
    for (int i0 = 0; i0 < a->n; i0 += a->per_launch) {
        const int c = std::min(a->per_launch, a->n - i0);
        const long long len = tail + (long long)c * a->H;
        double* const nl = a->line[a->cur ^ 1];
        hipLaunchKernelGGL(bbspec_line_kernel, dim3((unsigned)((len + BS_T - 1) / BS_T), (a->Mv + BS_T - 1) / BS_T, sets), dim3(256), 0, s,
                           a->p + (size_t)i0 * a->H * a->Mv, a->p_set, a->line[a->cur], a->len, nl, len, tail, a->Mv);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        a->cur ^= 1;
        a->len = len;
        const void* x[1] = {nl};
        void* spec[1] = {a->spec};
        const int n_ch[1] = {sets * a->Mv};
        const long stride_c[1] = {1}, stride_k[1] = {(long)sets * a->Mv}, spec_hop[1] = {(long)K * sets * a->Mv};
        e = apv_launch_stft_analysis_chunk(1, a->N, 1, x, n_ch, spec, stride_c, stride_k, (long)len, a->H, spec_hop, c, s, why);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bbspec_energy_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s,
                           static_cast<const double2*>(a->spec), a->totals, a->Z, a->E, K, a->Mv, c);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (a->detect) {
            // on this sub-launch's spectra, before the next one overwrites them
            e = bbspec_detect(*a->detect, a->spec, i0, c, a->N, a->Z, a->E, a->Mv, s, why);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}
