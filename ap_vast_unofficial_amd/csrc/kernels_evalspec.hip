// Per-bin evaluation spectra of the subband stream (apv_stream_set_evaluation_spectra): behind the evaluation stage of a hop
// (kernels_streameval.hip), the pressures p [sets][H][Mv] it left are framed with the stream's block N and hop H, windowed,
// transformed, and |P|^2 is accumulated per bin.  With f_t[s][i, m] = p[s][(t + 1) H - N + i, m] the frame after hop t (zero
// before sample 0), w the stream's sine window and P_t[s][k, m] = rfft(w f_t[s][:, m])[k], k < K = N/2 + 1, unnormalised:
//
//   bright[z, v, m, k] += |P_bright|^2        dark[z, v, m, k] += |P_dark|^2
//   error [z, v, m, k] += |P_target - P_bright|^2        target[z, m, k] += |P_target|^2
//
// Three launches, everything float64:
//
// 1. eval_ring_kernel.  The hop's pressures [sets][H][Mv] (microphones contiguous) into the pressure ring [sets Mv][N] (samples
// contiguous), a channel-major ring like the response rings of K1 and with the stream's ring offset: sample i of the hop goes to
// (N - H + i + ring_off) mod N, so the hop wraps inside the ring whenever H does not divide N.  A transposition: a workgroup
// moves a tile of 16 samples x 16 microphones through LDS (rows padded to 17), reading runs of 16 microphones (128 bytes, two
// whole lines where the row is aligned) and writing runs of 16 samples.
//
// 2. The stream's own analysis launch (apv_launch_stft_analysis_jobs, float64) on the ring: ONE channel set of sets Mv channels,
// windowed, into the bin-major scratch spec [K][sets Mv] complex128.  Every even N the stream accepts in float64, Bluestein sizes
// included, with no second FFT.
//
// 3. eval_energy_kernel.  One thread per (zone program, bin, microphone), microphones fastest as in the scratch: it reads the
// target's bin once and, per evaluated rank, bright and dark, and adds the four squared magnitudes to the totals
// [Z][3 E + 1][K][Mv] (per program: bright of the E ranks, dark, error, target), total = total + hop.  The error spectrum is
// P_target - P_bright by linearity.  No atomics: one thread owns an element, so the bits depend on the data alone.
//
// Bounds: every access of 1 and 3 is predicated; H, Mv, N need not be multiples of anything.  Nothing is read past
// [sets][H][Mv] pressures and [K][sets Mv] spectra, nothing written past [sets Mv][N] ring samples and [Z][3 E + 1][K][Mv] totals.
#include "apv_internal.h"

namespace {

constexpr int ES_T = 16;                       // tile edge: 16 samples x 16 microphones, one element per thread

__global__ void __launch_bounds__(256) eval_ring_kernel(const double* __restrict__ p, double* __restrict__ ring, int H, int Mv, int N,
                                                        int ring_off) {
    __shared__ double tile[ES_T][ES_T + 1];
    const int set = blockIdx.z, n0 = blockIdx.x * ES_T, m0 = blockIdx.y * ES_T;
    const int a = threadIdx.x >> 4, b = threadIdx.x & 15;
    // in: neighbouring threads along the microphones
    if (n0 + a < H && m0 + b < Mv) tile[a][b] = p[((size_t)set * H + n0 + a) * Mv + m0 + b];
    __syncthreads();
    // out: neighbouring threads along the samples
    const int m = m0 + a, n = n0 + b;
    if (m < Mv && n < H) {
        int pos = N - H + n + ring_off;        // < 2 N: ring_off < N, n < H <= N
        if (pos >= N) pos -= N;
        ring[((size_t)set * Mv + m) * N + pos] = tile[b][a];
    }
}

__global__ void __launch_bounds__(256) eval_energy_kernel(const double2* __restrict__ spec, double* __restrict__ totals, int Z, int E,
                                                          int K, int Mv) {
    const size_t items = (size_t)Z * K * Mv, it = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (it >= items) return;
    const int m = (int)(it % Mv), k = (int)((it / Mv) % K), z = (int)(it / ((size_t)Mv * K));
    const size_t row = (size_t)Z * (2 * E + 1) * Mv;                  // channels of one bin of the scratch
    const double2* __restrict__ sz = spec + (size_t)k * row + (size_t)z * (2 * E + 1) * Mv + m;
    double* __restrict__ tz = totals + ((size_t)z * (3 * E + 1) * K + k) * Mv + m;
    const size_t plane = (size_t)K * Mv;
    const double2 t = sz[(size_t)2 * E * Mv];
    for (int e = 0; e < E; ++e) {
        const double2 br = sz[(size_t)e * Mv], dk = sz[(size_t)(E + e) * Mv];
        const double dx = t.x - br.x, dy = t.y - br.y;
        tz[(size_t)e * plane] = tz[(size_t)e * plane] + (br.x * br.x + br.y * br.y);
        tz[(size_t)(E + e) * plane] = tz[(size_t)(E + e) * plane] + (dk.x * dk.x + dk.y * dk.y);
        tz[(size_t)(2 * E + e) * plane] = tz[(size_t)(2 * E + e) * plane] + (dx * dx + dy * dy);
    }
    tz[(size_t)3 * E * plane] = tz[(size_t)3 * E * plane] + (t.x * t.x + t.y * t.y);
}

}  // namespace

bool apv_eval_spectra_size_ok(int N, int H, int Z, int E, int Mv, std::string* why) {
    if (N < 4 || (N & 1) || N > 4096) {
        if (why) *why = "evaluation spectra: the float64 transforms take even block sizes in 4..4096";
        return false;
    }
    if (H < 1 || H > N || Z < 1 || Z > 2 || E < 1 || Mv < 1) {
        if (why) *why = "evaluation spectra: H in 1..N, Z in 1..2, E and Mv at least 1";
        return false;
    }
    const size_t sets = (size_t)Z * (2 * (size_t)E + 1);
    if (sets > 65535 || ((size_t)Mv + ES_T - 1) / ES_T > 65535 || sets * Mv > 0x7fffffffull ||
        ((size_t)Z * (N / 2 + 1) * Mv + 255) / 256 > 0x7fffffffull) {
        if (why) *why = "evaluation spectra: at most 65535 pressure sets, 16 x 65535 microphones and 2^31 - 1 transforms per hop";
        return false;
    }
    return apv_stft_size_ok(N, why);
}

hipError_t apv_launch_eval_spectra(const EvalSpectraArgs& a, hipStream_t s, std::string* why) {
    if (!apv_eval_spectra_size_ok(a.N, a.H, a.Z, a.E, a.Mv, why)) return hipErrorInvalidValue;
    if (!a.p || !a.ring || !a.spec || !a.totals || a.ring_off < 0 || a.ring_off >= a.N) {
        if (why) *why = "evaluation spectra: null device pointer or ring offset outside 0..N - 1";
        return hipErrorInvalidValue;
    }
    const int sets = a.Z * (2 * a.E + 1), K = a.N / 2 + 1;
    hipLaunchKernelGGL(eval_ring_kernel, dim3((a.H + ES_T - 1) / ES_T, (a.Mv + ES_T - 1) / ES_T, sets), dim3(256), 0, s, a.p, a.ring,
                       a.H, a.Mv, a.N, a.ring_off);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const void* x[1] = {a.ring};
    void* spec[1] = {a.spec};
    const int n_ch[1] = {sets * a.Mv};
    const long stride_c[1] = {1}, stride_k[1] = {(long)sets * a.Mv};
    e = apv_launch_stft_analysis_jobs(1, a.N, 1, x, n_ch, spec, stride_c, stride_k, a.ring_off, s, why);
    if (e != hipSuccess) return e;
    const size_t items = (size_t)a.Z * K * a.Mv;
    hipLaunchKernelGGL(eval_energy_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s,
                       static_cast<const double2*>(a.spec), a.totals, a.Z, a.E, K, a.Mv);
    return hipGetLastError();
}
