// Broadband (time-domain) AP-VAST on the device, float64: the reference's own algorithm, stage by stage.
//
//   apv_bb_init          allocate state, upload RIRs                       reference Python/apvast.py:97-151
//   apv_bb_process_block one hop                                            apvast.py:153-165
//     1 RIR convolution into the response rings                             apvast.py:167-194
//     2 WOLA of target / response rings (weights = 1), head of the overlap
//       buffers appended to the statistics rings                            apvast.py:197-311
//     3 R = sum_m Y_m Y_m^T, r = sum_m Y_m d_m from the statistics rings,
//       Y the data matrix of apvast.py:334-338 INCLUDING the sample that
//       scipy.linalg.toeplitz drops                 apvast.py:329-364
//     4 jdiag + rank-accumulated filters (apv_gevd_large)                   apvast.py:378-414
//     5 filter spectra = rfft(taps, N)                                      apvast.py:417-422
//     6 input spectra x filter spectra, inverse STFT, window, overlap-add   apvast.py:428-506
//
// Host code only: the stream's kernels are in kernels_bb.hip and kernels_norm2.hip, behind apv_launch_* (apv_internal.h).
//
// Channel order on the device: c = m*L + l (as in stream.hip).  Everything is double: the dark matrix is loaded
// with an ABSOLUTE 1e-7 (apvast.py:23) against entries of order 1e-3, so float statistics would not survive.
#include "apv_internal.h"
#include "apv_owned.h"
#include "state_layout.h"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>

#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

struct apv_bb {
    int N, H, K, L, M, C, P, J, S, V, n, zones, pad;      // V = number of solutions (ranks kept)
    int dialect, skip, ncols, toff, rel_loading, rel_dark_py;          // statistics conventions of the dialect
    long not_converged;    // hops whose joint diagonalisation hit the sweep cap
    int* d_ranks;          // [V] ascending
    int max_rank;          // the largest of them: the eigenpairs a hop consumes (apvast.py:406-414)
    int full_valid;        // U / lam hold ALL eigenpairs of the last hop (0: the leading block only; the rest is computed when read)
    double* nrm;           // [4] ||R_q||_2 for the relative loading
    int ring_off, stat_off, cur;
    int n_out;
    double* rir[2];        // [P][C]
    double* trir[2];       // [P][M]
    double* xhist[2][2];   // [buf][signal][P-1+H+pad]
    double* xin;           // [2][H]
    double* resp[4];       // [C][N] rings
    double* tresp[2];      // [M][N] rings
    double* inblk;         // [2][N] rings
    double* spec;          // scratch spectra [max(C, n_out)][K] c128
    double* ov[4];         // [C][N] overlap buffers of the weighted responses (linear, shifted by the kernel)
    double* tov[2];        // [M][N]
    double* stats[4];      // [C][S] rings
    double* tstats[2];     // [M][S] rings
    double* R;             // [4][n][n]: bright AA, BB, then dark AB, BA (zone A = (0, 2), zone B = (1, 3))
    double* r;             // [2][n]
    double* U;             // [2][n][n]
    double* lam;           // [2][n]
    double* w;             // [2][V][n]
    double* fspec;         // [n_out][K] c128 filter spectra (zone A ranks, zone B ranks, target A, target B)
    double* inspec;        // [2][K] c128
    double* outov;         // [n_out][N]
    double* out;           // [n_out][H]
    // perceptual weighting (off when nch == 0)
    int nch, norm_mode;
    double Cs, Ca, Leff;
    double* G2;            // [K][nch]
    double* G2T;           // [nch][K]
    double* tspec[2];      // [M][K] c128 target spectra (kept: the curves come from both zones before any scaling)
    // Round 4: the four response sets and the two target sets of a hop are ONE set of 4 C + 2 M channels -- rings, overlap buffers,
    // statistics rings and spectra are each one allocation, paths first, then the targets (resp[p], tresp[z], ov[p], ... point into
    // them) -- so that the hop's windowed transforms, its synthesis and its append to the statistics rings are one launch each
    // instead of six (apvast.py:197-311 runs the same three steps per buffer).
    double *resp_all, *ov_all, *stats_all, *pspec_all;
    // pinned staging of the per-hop call (round 4): the caller's arrays are pageable, and an asynchronous copy from / to pageable
    // memory is staged by the runtime behind a synchronisation of its own -- 83 us between the last kernel of a hop and the start
    // of its copy back in the trace.  The hop's inputs are copied here first and its outputs land here.
    double* pin_in;        // [2][H]
    double* pin_out;       // [n_out][H]
    int n_all;             // 4 C + 2 M
    double* Wgt[2];        // [M][K]
    // apv_bb_process_signal: G consecutive hops share ONE batched joint diagonalisation (allocated on first use)
    int grp;               // hops per group the buffers below are sized for (0: not allocated)
    double* g_xin;         // [grp][2][H] the group's input hops
    double* g_RA;          // [grp * nz][n][n] bright matrices, (hop, zone that runs) major
    double* g_RB;          // [grp * nz][n][n] dark matrices
    double* g_U;           // [grp * nz][n][n]
    double* g_lam;         // [grp * nz][n]
    double* g_r;           // [grp * nz][n]
    double* g_w;           // [grp * nz][V][n]
    double* g_nrm;         // [grp][4] + [grp * nz] dark norms in batch order
    double* g_inspec;      // [grp][2][K] c128
    double* g_out;         // [2 sets] a group's output hops as the caller's array holds them: [n_out / L][grp H][L] with
                           // cfg.out_layout = 1, else [grp][n_out][H]: ONE copy per group to the host
    double* g_pin;         // [2 sets] the same, page-locked: staging for a caller's pageable array (allocated when first needed)
    size_t g_pin_cap;      // doubles per set g_pin holds
    double* g_pin_in;      // [2 sets][grp][2][H] page-locked: a group's input hops, gathered here and sent in ONE copy
    int out_group;         // cfg.out_layout = 1: L (sample-major emit, see bb_back); 0: channel-major
    // (each of the above twice: the front stages of group g + 1 fill one set while the batched solve of group g reads the other)
    double* spec_out;      // [n_out][K] c128: the output stage's own spectra (the front stages use `spec` at the same time)
    hipStream_t front;     // the front stages of apv_bb_process_signal
    hipStream_t copy;      // a group's outputs on their way to the host while the next group is solved
    hipStream_t front2;    // the statistics of hop h beside the K1 / WOLA chain of hop h + 1 (apv_bb_process_signal)
    hipEvent_t ev_ring, ev_stat;             // hop's statistics rings written / read
    hipEvent_t ev_front[2], ev_back[2];      // group set filled / group set read for the last time
    hipEvent_t ev_out[2];                    // a group's outputs have reached g_pin
    FirLive live;          // responses reassigned between hops (apv_bb_set_rirs): the correction tails still to be added to K1's output
    // evaluation stage (apv_bb_set_evaluation, kernels_bbeval.hip); be_on = 0: off, nothing below exists
    std::vector<int> rank_vals;   // the ranks of the V solutions, as d_ranks holds them
    int be_on;
    int be_Pv, be_Mv, be_E, be_Z; // response taps, validation microphones, evaluated ranks, zone programs that run
    int be_sets, be_nhist;        // pressure sets be_Z (2 be_E + 1), evaluated groups be_Z (be_E + 1)
    int be_cur;                   // the history buffer the next launch reads
    double* be_rv[2];             // [Pv][L][Mv] responses to the validation microphones of zone A, zone B
    int32_t* be_map;              // [sets][4] {group of the emitted hop, history slot, bank, -} of every pressure set
    int32_t* be_hsrc;             // [nhist] the group behind every history slot
    double* be_hist[2];           // [nhist][Pv - 1][L], alternating
    double* be_p;                 // [sets][be_p_hops H][Mv]; a launch over c hops fills [sets][c H][Mv] of it
    int be_p_hops, be_last;       // hops the pressure buffer holds per set; hops of the last launch (0: none yet)
    double* be_tot;               // [Z][3 E + 1][Mv]
    double* be_rec;               // [be_cap] slots of [Z][3 E + 1][Mv]: the energies of every hop of the last call
    int be_cap, be_nrec;          // slots allocated; slots the last call filled
    // per-bin spectra of that stage (apv_bb_set_evaluation_spectra, kernels_bbevalspec.hip); bs_on = 0: off, nothing below exists
    int bs_on;
    int bs_hops, bs_cur;          // hops of a sub-launch the line buffers and the scratch hold; the buffer with the current line
    long long bs_len;             // samples per channel of the current line, at least N: its last N are "eval_ring"
    double* bs_line[2];           // [sets Mv][N - H + bs_hops H], alternating
    void* bs_spec;                // [bs_hops][K][sets Mv] complex128, the transforms' bin-major scratch
    double* bs_tot;               // [Z][3 E + 1][K][Mv]
    // perceptual detectability behind those spectra (apv_bb_set_evaluation_detectability, kernels_evaldetect.hip, hop-batched);
    // bd_on = 0: off, nothing below exists
    int bd_on;
    int bd_C;                     // channels of the model
    double bd_Cs, bd_Ca, bd_Leff;
    double* bd_G2T;               // [bd_C][K]: the squared channel responses, channel-major
    double* bd_quiet;             // [K]: the curve of a silent masker (read with one zone program), formed once
    double* bd_curves;            // [bs_hops][K][Z Mv]: the squared weighting curves of a sub-launch's hops
    double* bd_part;              // [bs_hops][chunks][Z][2 E][Mv]: their partial sums
    double* bd_tot;               // [Z][6 E][Mv]: per program sum, max and count of D > 1 of the error, then of the leak
    double* bd_rec;               // [bd_cap] slots of [Z][2 E][Mv]: the values of every hop of the last call
    int bd_cap, bd_nrec;          // slots allocated; slots the last call filled
    ApvOwned own;         // every buffer, pinned block, event and stream above: made through it, freed by it
};

namespace {

#define BCHK(h, call)                                                                    \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess) return apv_fail(h, APV_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_e)); \
    } while (0)

// true when [p, p + bytes) lies in page-locked host memory: a device-to-host copy into it is a DMA that runs asynchronously; any
// other host pointer is staged by the runtime and blocks the caller.  Blocks of apv_host_alloc are known without asking the
// runtime; with `ask` any other pointer is looked up there (a search and, for pageable memory, an error path: once per whole
// signal, never per hop).
bool host_is_pinned(const void* p, size_t bytes, bool ask) {
    if (apv_host_block_contains(p, bytes)) return true;
    if (!ask) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// dst[r][0 : width] = src[r][0 : width], r < rows (pitches in doubles), shared out over a few threads: the collection of a group
// of hops from the staging buffer into the caller's pageable array runs at memory speed, not at one core's
void copy_rows(double* dst, size_t dpitch, const double* src, size_t spitch, size_t width, size_t rows) {
    const size_t total = width * rows * sizeof(double);
    const unsigned hw = std::thread::hardware_concurrency();
    size_t nt = total >> 21;                            // a thread per 2 MiB
    nt = nt < 1 ? 1 : (nt > 8 ? 8 : nt);
    if (hw && nt > hw) nt = hw;
    // rows are split in pieces when there are fewer rows than threads
    const size_t pieces = rows >= nt ? 1 : (nt + rows - 1) / rows;
    const size_t units = rows * pieces, pw = (width + pieces - 1) / pieces;
    auto work = [&](size_t t) {
        for (size_t u = t; u < units; u += nt) {
            const size_t r = u / pieces, c0 = (u % pieces) * pw;
            if (c0 >= width) continue;
            const size_t w = width - c0 < pw ? width - c0 : pw;
            std::memcpy(dst + r * dpitch + c0, src + r * spitch + c0, w * sizeof(double));
        }
    };
    if (nt == 1) return work(0);
    std::vector<std::thread> th;
    for (size_t t = 1; t < nt; ++t) th.emplace_back(work, t);
    work(0);
    for (auto& x : th) x.join();
}

// `count` doubles, zeroed, kept by the stream
int dalloc(apv_handle* h, double** p, size_t count) {
    BCHK(h, h->bb->own.zeroed(p, count, sizeof(double), h->stream));
    return APV_OK;
}

// Which zone programs run (cfg.n_zones: bit 0 = A, bit 1 = B) and what of a hop belongs to each.  Two index conventions meet here
// and nowhere else:
//   paths    p = 0..3: A->A, A->B, B->A, B->B: signal p >> 1 through the responses of zone p & 1 (resp, ov, stats, pspec).  Zone
//            program A shapes signal A, so it owns paths 0 and 1; a program that does not run leaves its paths' spectra at zero
//            (apvast.py:239-255).
//   matrices i = 0..3: bright A->A, B->B, then dark A->B, B->A (R, nrm): zone program i & 1, bright i < 2.
// A batch of the solver holds the zones that run side by side, hop-major: zone z sits in slot z - first of its hop's nz.
struct BbZones {
    bool run[2];
    int first, nz;         // the first zone program that runs and how many do
    explicit BbZones(int mask) : run{(mask & 1) != 0, (mask & 2) != 0}, first(run[0] ? 0 : 1), nz(run[0] && run[1] ? 2 : 1) {}
    static int path_sig(int p) { return p >> 1; }
    static int path_zone(int p) { return p & 1; }
    bool path_live(int p) const { return run[path_sig(p)]; }
    bool mat_live(int i) const { return run[i & 1]; }
    static int mat_path(int i) { return i < 2 ? 3 * i : i - 1; }        // the statistics path behind matrix i: 0, 3, 1, 2
    int slot(int z) const { return z - first; }
    // the matrix whose norm stands in entry i of a hop's four: itself, or for a program that does not run the other's of its kind
    int norm_src(int i) const { return mat_live(i) ? i : ((i & 2) | first); }
    int first_dark() const { return 2 + first; }                        // the dark matrix of the first zone that runs
};

// wall time since the last call (or construction), in ms: APV_BB_TIMING
struct WallTimer {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap() {
        const auto now = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(now - t).count();
        t = now;
        return ms;
    }
};
// APV_BB_TIMING=1: synchronise at the stage boundaries and print the wall time of each (profiling aid; rocprofv3 cannot trace the
// per-hop path)
bool bb_timing() {
    static const bool on = getenv("APV_BB_TIMING") != nullptr;
    return on;
}

}  // namespace

void apv_bb_free(apv_handle* h) {
    apv_bb* s = h->bb;
    if (!s) return;
    apv_live_free(s->live);
    delete s;
    h->bb = nullptr;
}

extern "C" {

// Ranks of the solutions the next apv_bb_init keeps (apVast.m:527-549 takes a vector of ranks); n_ranks = 0 restores
// "every rank 1..number_of_eigenvectors" (apvast.py:406-422).
int apv_bb_set_rank_list(apv_handle* h, int32_t n_ranks, const int32_t* ranks) {
    if (!h || n_ranks < 0 || (n_ranks > 0 && !ranks)) return apv_fail(h, APV_ERR_ARG, "bad rank list");
    h->bb_rank_list.assign(ranks, ranks + n_ranks);
    return APV_OK;
}

int apv_bb_init(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B,
                int32_t reference_index_A, int32_t reference_index_B, int32_t modeling_delay,
                int32_t filter_length, int32_t statistics_buffer_length, int32_t number_of_eigenvectors) {
    if (!h || !h_rir_A || !h_rir_B) return apv_fail(h, APV_ERR_ARG, "null argument");
    if (h->span.on) return apv_fail(h, APV_ERR_ARG, "broadband mode: the handle has a span (apv_set_span), a subband feature");
    if (h->effort.on) return apv_fail(h, APV_ERR_ARG, "broadband mode: the handle has an effort limit (apv_stream_set_effort_limit), a subband feature");
    if (h->valspan.on) return apv_fail(h, APV_ERR_ARG, "broadband mode: the handle has a validation span (apv_stream_set_validation_span), a subband feature");
    const apv_config& c = h->cfg;
    const int N = c.block_size, H = c.hop_size, J = filter_length, S = statistics_buffer_length;
    const int V = number_of_eigenvectors, L = c.n_srcs, M = c.n_mics;
    {
        std::string why;
        if (!apv_stft_size_ok(N, &why)) return apv_fail(h, APV_ERR_ARG, why);
    }
    if (N > 4096) return apv_fail(h, APV_ERR_ARG, "broadband mode: block_size <= 4096 (double-precision FFT in LDS)");
    if (H < 1 || H > N) return apv_fail(h, APV_ERR_ARG, "hop_size must be in 1..block_size");
    if (J < 1 || J > N || S <= J + 1 || H > S) return apv_fail(h, APV_ERR_ARG, "need 1 <= filter_length <= block_size and statistics_buffer_length > filter_length + 1, >= hop_size");
    const int n = J * L;
    if (n > 4096) return apv_fail(h, APV_ERR_ARG, "broadband mode: filter_length * loudspeakers <= 4096");
    if (V < 1 || V > n) return apv_fail(h, APV_ERR_ARG, "number_of_eigenvectors must be in 1..filter_length*loudspeakers");
    // ranks kept: every rank 1..V (apvast.py:406-422) unless a list was registered (apVast.m:527-549)
    std::vector<int> ranks = h->bb_rank_list;
    if (ranks.empty())
        for (int v = 1; v <= V; ++v) ranks.push_back(v);
    for (size_t i = 0; i < ranks.size(); ++i)
        if (ranks[i] < 1 || ranks[i] > n || (i && ranks[i] <= ranks[i - 1]))
            return apv_fail(h, APV_ERR_ARG, "rank list must be ascending and within 1..filter_length*loudspeakers");
    const int dialect = c.dialect;
    if (dialect != APV_DIALECT_PYTHON && dialect != APV_DIALECT_MATLAB) return apv_fail(h, APV_ERR_ARG, "unknown dialect");
    if (rir_len < 1 || modeling_delay < 0 || modeling_delay >= rir_len || modeling_delay >= J)
        return apv_fail(h, APV_ERR_ARG, "modeling_delay must be < rir_len and < filter_length");
    if (reference_index_A < 0 || reference_index_A >= L || reference_index_B < 0 || reference_index_B >= L)
        return apv_fail(h, APV_ERR_ARG, "reference index out of range");
    if (c.n_zones < 1 || c.n_zones > 3) return apv_fail(h, APV_ERR_ARG, "n_zones is a bit mask: 1 = A, 2 = B, 3 = both");
    BCHK(h, hipSetDevice(h->device));
    apv_bb_free(h);
    apv_bb* s = new apv_bb();                               // value-initialised: every scalar, pointer and array member starts at zero
    h->bb = s;
    // an init that fails from here on leaves no half-built stream behind
    struct Guard { apv_handle* h; bool ok; ~Guard() { if (!ok) apv_bb_free(h); } } built{h, false};
    const int nsol = (int)ranks.size();
    s->N = N; s->H = H; s->K = N / 2 + 1; s->L = L; s->M = M; s->C = L * M; s->P = rir_len; s->J = J; s->S = S; s->V = nsol;
    s->n = n; s->zones = c.n_zones; s->pad = apv_fir_pad_f64();
    s->dialect = dialect;
    s->skip = dialect == APV_DIALECT_PYTHON;                 // scipy's toeplitz drops sample J (apvast.py:336-338)
    s->ncols = S - J + (s->skip ? 0 : 1);                    // apvast.py:334 / apVast.m:420
    s->toff = s->skip ? J : J - 1;                           // apvast.py:340 d[J:] / apVast.m:425 d(J:end)
    s->rel_loading = c.reg_mode == APV_REG_REL && dialect == APV_DIALECT_MATLAB;      // apVast.m:552-569, in place
    s->rel_dark_py = c.reg_mode == APV_REG_REL && dialect == APV_DIALECT_PYTHON;      // apvast.py:26-27, inside jdiag
    const int nz = BbZones(s->zones).nz;
    s->n_out = nz * nsol * L + 2 * L;
    s->out_group = c.out_layout == 1 ? L : 0;
    s->max_rank = ranks.back();
    s->rank_vals = ranks;
    s->full_valid = 1;
    BCHK(h, s->own.device(&s->d_ranks, sizeof(int) * nsol));
    BCHK(h, hipMemcpyAsync(s->d_ranks, ranks.data(), sizeof(int) * nsol, hipMemcpyHostToDevice, h->stream));
    BCHK(h, hipStreamSynchronize(h->stream));
    const int C = s->C, P = s->P, K = s->K;
    int rc;
    std::vector<double> tmp((size_t)P * C), ttmp((size_t)P * M);
    for (int z = 0; z < 2; ++z) {
        const double* src = z ? h_rir_B : h_rir_A;
        const int ref = z ? reference_index_B : reference_index_A;
        for (int p = 0; p < P; ++p)
            for (int l = 0; l < L; ++l)
                for (int m = 0; m < M; ++m) tmp[(size_t)p * C + m * L + l] = src[((size_t)p * L + l) * M + m];
        std::fill(ttmp.begin(), ttmp.end(), 0.0);
        for (int p = modeling_delay; p < P; ++p)
            for (int m = 0; m < M; ++m) ttmp[(size_t)p * M + m] = src[((size_t)(p - modeling_delay) * L + ref) * M + m];
        if ((rc = dalloc(h, &s->rir[z], (size_t)P * C))) return rc;
        if ((rc = dalloc(h, &s->trir[z], (size_t)P * M))) return rc;
        // on the handle's stream, behind the zero-fill of dalloc (a null-stream hipMemcpy is not ordered with it)
        BCHK(h, hipMemcpyAsync(s->rir[z], tmp.data(), sizeof(double) * tmp.size(), hipMemcpyHostToDevice, h->stream));
        BCHK(h, hipMemcpyAsync(s->trir[z], ttmp.data(), sizeof(double) * ttmp.size(), hipMemcpyHostToDevice, h->stream));
        BCHK(h, hipStreamSynchronize(h->stream));           // tmp / ttmp are rewritten for the next zone
    }
    const size_t hist = (size_t)P - 1 + H + s->pad;
    for (int b = 0; b < 2; ++b)
        for (int g = 0; g < 2; ++g)
            if ((rc = dalloc(h, &s->xhist[b][g], hist))) return rc;
    if ((rc = dalloc(h, &s->xin, (size_t)2 * H))) return rc;
    s->n_all = 4 * C + 2 * M;
    if ((rc = dalloc(h, &s->resp_all, (size_t)s->n_all * N))) return rc;
    if ((rc = dalloc(h, &s->ov_all, (size_t)s->n_all * N))) return rc;
    if ((rc = dalloc(h, &s->stats_all, (size_t)s->n_all * S))) return rc;
    if ((rc = dalloc(h, &s->pspec_all, (size_t)s->n_all * K * 2))) return rc;
    for (int p = 0; p < 4; ++p) {
        s->resp[p] = s->resp_all + (size_t)p * C * N;
        s->ov[p] = s->ov_all + (size_t)p * C * N;
        s->stats[p] = s->stats_all + (size_t)p * C * S;
    }
    for (int z = 0; z < 2; ++z) {
        s->tresp[z] = s->resp_all + ((size_t)4 * C + (size_t)z * M) * N;
        s->tov[z] = s->ov_all + ((size_t)4 * C + (size_t)z * M) * N;
        s->tstats[z] = s->stats_all + ((size_t)4 * C + (size_t)z * M) * S;
        s->tspec[z] = s->pspec_all + ((size_t)4 * C + (size_t)z * M) * K * 2;
    }
    const size_t spec_ch = (size_t)(C > s->n_out ? C : s->n_out);
    if ((rc = dalloc(h, &s->spec, spec_ch * K * 2))) return rc;
    if ((rc = dalloc(h, &s->inblk, (size_t)2 * N))) return rc;
    if ((rc = dalloc(h, &s->R, (size_t)4 * n * n))) return rc;
    if ((rc = dalloc(h, &s->r, (size_t)2 * n))) return rc;
    if ((rc = dalloc(h, &s->U, (size_t)2 * n * n))) return rc;
    if ((rc = dalloc(h, &s->lam, (size_t)2 * n))) return rc;
    if ((rc = dalloc(h, &s->w, (size_t)2 * nsol * n))) return rc;
    if ((rc = dalloc(h, &s->nrm, 4))) return rc;
    if ((rc = dalloc(h, &s->fspec, (size_t)s->n_out * K * 2))) return rc;
    if ((rc = dalloc(h, &s->inspec, (size_t)2 * K * 2))) return rc;
    if ((rc = dalloc(h, &s->outov, (size_t)s->n_out * N))) return rc;
    if ((rc = dalloc(h, &s->out, (size_t)s->n_out * H))) return rc;
    BCHK(h, s->own.pinned(&s->pin_in, sizeof(double) * 2 * H));
    BCHK(h, s->own.pinned(&s->pin_out, sizeof(double) * (size_t)s->n_out * H));
    // target filter spectra: the Python class uses the zone-A reference for both A_t and B_t (apvast.py:389-390, 418,
    // 422), the MATLAB class one reference per zone (apVast.m:597-602)
    std::vector<double> tg((size_t)2 * L * K * 2, 0.0);
    const double PI = 3.14159265358979323846;
    for (int z = 0; z < 2; ++z)
        for (int k = 0; k < K; ++k) {
            const double ph = -2.0 * PI * (double)k * (double)modeling_delay / (double)N;
            const int ref = (z == 1 && dialect == APV_DIALECT_MATLAB) ? reference_index_B : reference_index_A;
            const size_t o = (((size_t)z * L + ref) * K + k) * 2;
            tg[o] = std::cos(ph);
            tg[o + 1] = std::sin(ph);
        }
    BCHK(h, hipMemcpyAsync(s->fspec + (size_t)nz * nsol * L * K * 2, tg.data(), sizeof(double) * tg.size(), hipMemcpyHostToDevice,
                           h->stream));
    BCHK(h, apv_stft_prepare(N, 1));
    BCHK(h, hipStreamSynchronize(h->stream));
    built.ok = true;
    return APV_OK;
}

// Where one hop's statistics and solution live: the handle's own arrays for apv_bb_process_block, slices of the group buffers
// for apv_bb_process_signal.
struct BbHop {
    const double* xin;     // [2][H] the hop's input samples (device)
    double* Rq[4];         // bright A->A, B->B; dark A->B, B->A (zones that do not run: unused)
    double* r[2];          // per zone
    double* nrm;           // [4] ||R_q||_2
    double* nrm_dark;      // first dark norm in the order the batch holds the matrices (relative loading of the Python dialect)
    double* inspec;        // [2][K] c128
    double* w[2];          // per zone [V][n]
};

static BbHop bb_own_hop(apv_bb* s) {
    const size_t nn = (size_t)s->n * s->n;
    BbHop q{};
    q.xin = s->xin;
    for (int i = 0; i < 4; ++i) q.Rq[i] = s->R + i * nn;
    for (int z = 0; z < 2; ++z) {
        q.r[z] = s->r + (size_t)z * s->n;
        q.w[z] = s->w + (size_t)z * s->V * s->n;
    }
    q.nrm = s->nrm;
    q.nrm_dark = s->nrm + BbZones(s->zones).first_dark();
    q.inspec = s->inspec;
    return q;
}

// Stage 4: jdiag + filters of `batch` pairs lying one behind the other; w == nullptr: every eigenpair and no filters (the
// attributes lambda_* / U_* read after a hop that solved for the leading eigenpairs only).  The one place that knows how the dialect
// loads the dark matrix: the MATLAB dialect has loaded it in place (front_statistics), the Python dialect lets jdiag load a copy --
// with reg_dark, or with EXPERIMENTAL_REGULARIZATION = False with reg_dark ||B||_2 from nrm_dark (apvast.py:26-27); the R_*
// attributes stay as accumulated.
static int bb_solve(apv_handle* h, apv_bb* s, const double* A, const double* B, const double* nrm_dark, double* U, double* lam,
                    const double* r, double* w, int batch, int32_t* status) {
    h->gl_lead_rank = w ? s->max_rank : 0;
    return apv_gevd_large(h, s->n, batch, A, B, s->rel_loading ? 0.0 : h->cfg.reg_dark, s->rel_dark_py ? nrm_dark : nullptr, U, lam, r,
                          h->cfg.mu, w ? s->V : 0, w ? s->d_ranks : nullptr, w, status);
}

// the same on the handle's own arrays: the zone programs that run are one batch
static int bb_solve_own(apv_handle* h, apv_bb* s, bool filters, int32_t status[2]) {
    const BbZones zn(s->zones);
    const size_t n = s->n, nn = n * n, f = zn.first;
    return bb_solve(h, s, s->R + f * nn, s->R + zn.first_dark() * nn, s->nrm + zn.first_dark(), s->U + f * nn, s->lam + f * n,
                    filters ? s->r + f * n : nullptr, filters ? s->w + f * s->V * n : nullptr, zn.nz, status);
}

// new input histories, the ring offsets of this hop, and the hop appended to the ring of input blocks
static int front_history_and_rings(apv_handle* h, apv_bb* s, const BbHop& q, hipStream_t st) {
    const int nxt = s->cur ^ 1;
    BCHK(h, apv_launch_hist2_f64(s->P, s->H, s->pad, s->xhist[s->cur][0], s->xhist[s->cur][1], q.xin, s->xhist[nxt][0],
                                 s->xhist[nxt][1], st));
    s->cur = nxt;
    s->ring_off = (s->ring_off + s->H) % s->N;
    s->stat_off = (s->stat_off + s->H) % s->S;
    BCHK(h, apv_launch_ring_append_f64(s->N, s->H, s->ring_off, q.xin, (long)s->H, s->inblk, 2, st));
    return APV_OK;
}

// 1: RIR convolution into the response rings
static int front_k1(apv_handle* h, apv_bb* s, hipStream_t st) {
    const int C = s->C, M = s->M, P = s->P, H = s->H, N = s->N;
    FirJobsD jobs{};
    int nj = 0;
    for (int p = 0; p < 4; ++p) {
        jobs.rir[nj] = s->rir[BbZones::path_zone(p)]; jobs.xh[nj] = s->xhist[s->cur][BbZones::path_sig(p)]; jobs.resp[nj] = s->resp[p];
        jobs.C[nj++] = C;
    }
    for (int z = 0; z < 2; ++z) {
        jobs.rir[nj] = s->trir[z]; jobs.xh[nj] = s->xhist[s->cur][z]; jobs.resp[nj] = s->tresp[z];
        jobs.C[nj++] = M;
    }
    BCHK(h, apv_launch_fir_jobs_f64(jobs, nj, P, H, N, s->ring_off, st));
    if (s->live.hops_left > 0) {
        // responses replaced within the last P - 1 samples: the samples before the update ring out through the old ones
        double* dst[6] = {s->resp[0], s->resp[1], s->resp[2], s->resp[3], s->tresp[0], s->tresp[1]};
        const int rc = apv_live_apply(h, s->live, P, C, M, 1, (void* const*)dst, H, H, N, N - H + s->ring_off, N, st);
        if (rc != APV_OK) return rc;
        apv_live_advance(s->live, 1);
    }
    return APV_OK;
}

// 2: WOLA (unit weights, apvast.py:326-327, or the perceptual curves) into the overlap buffers: all 4 C + 2 M channels of the hop
// in one launch per step (see resp_all)
static int front_wola(apv_handle* h, apv_bb* s, hipStream_t st) {
    const int N = s->N, H = s->H, K = s->K, L = s->L, M = s->M, C = s->C;
    const BbZones zn(s->zones);
    std::string why;
    auto pspec = [&](int p) { return s->pspec_all + (size_t)p * C * K * 2; };
    BCHK(h, apv_launch_analysis(1, N, s->n_all, s->resp_all, N, N, s->ring_off, 1, s->pspec_all, K, 1, st, &why));
    for (int p = 0; p < 4; ++p)
        if (!zn.path_live(p)) BCHK(h, hipMemsetAsync(pspec(p), 0, sizeof(double) * 2 * (size_t)C * K, st));   // apvast.py:239-255: spectra stay 0
    if (s->nch > 0) {
        // curves from the unweighted target spectra of both zones (apvast.py:205), then the scaling (208-209);
        // A->A, B->A x zone A's curve; A->B, B->B x zone B's (apvast.py:258-262)
        for (int z = 0; z < 2; ++z)
            BCHK(h, apv_launch_perceptual_weights_f64(K, M, s->nch, (const double2*)s->tspec[z], s->G2, s->G2T, s->Cs, s->Ca,
                                                      s->Leff, N, s->norm_mode, s->Wgt[z], st));
        for (int z = 0; z < 2; ++z)
            BCHK(h, apv_launch_scale_spectra_cm_f64(K, M, 1, (double2*)s->tspec[z], s->Wgt[z], st));
        for (int p = 0; p < 4; ++p)
            if (zn.path_live(p)) BCHK(h, apv_launch_scale_spectra_cm_f64(K, C, L, (double2*)pspec(p), s->Wgt[BbZones::path_zone(p)], st));
    }
    BCHK(h, apv_launch_synthesis(1, N, H, s->n_all, s->pspec_all, K, 1, s->ov_all, nullptr, st, &why));
    return APV_OK;
}

// 3: R, r of the zone programs that run from the statistics rings, the dialect's scaling, the norms and the relative loading
static int front_statistics(apv_handle* h, apv_bb* s, const BbHop& q, hipStream_t st) {
    const int L = s->L, M = s->M, J = s->J, S = s->S, n = s->n;
    const BbZones zn(s->zones);
    const size_t nn = (size_t)n * n;
    SyrkJobs jobs{};
    int nj = 0;
    for (int i = 0; i < 4; ++i) {
        if (!zn.mat_live(i)) continue;
        jobs.stats[nj] = s->stats[BbZones::mat_path(i)];
        jobs.R[nj++] = q.Rq[i];
    }
    BCHK(h, apv_launch_syrk_hankel(st, n, J, L, M, S, s->stat_off, s->skip, s->ncols, nj, jobs));
    for (int z = 0; z < 2; ++z)
        if (zn.run[z])
            BCHK(h, apv_launch_xcorr_hankel(n, J, L, M, S, s->stat_off, s->skip, s->ncols, s->toff, s->stats[BbZones::mat_path(z)],
                                            s->tstats[z], q.r[z], st));
    if (s->dialect == APV_DIALECT_MATLAB) {
        // apVast.m:448-456: everything / ((S - J + 1) M)
        const double f = 1.0 / ((double)s->ncols * (double)M);
        for (int i = 0; i < 4; ++i)
            if (zn.mat_live(i)) BCHK(h, apv_launch_scale_f64(nn, q.Rq[i], f, st));
        for (int z = 0; z < 2; ++z)
            if (zn.run[z]) BCHK(h, apv_launch_scale_f64((size_t)n, q.r[z], f, st));
    }
    if (s->rel_loading || s->rel_dark_py) {
        const double* mats[4];
        for (int i = 0; i < 4; ++i) mats[i] = q.Rq[zn.norm_src(i)];
        BCHK(h, apv_launch_norm2(n, 4, mats, q.nrm, st));
        // the batch wants the dark norms of the zones that run side by side
        if (q.nrm_dark != q.nrm + zn.first_dark())
            BCHK(h, hipMemcpyAsync(q.nrm_dark, q.nrm + zn.first_dark(), sizeof(double) * zn.nz, hipMemcpyDeviceToDevice, st));
    }
    if (s->rel_loading) {
        // apVast.m:552-569: bright += reg_bright ||R||_2, dark += reg_dark ||R||_2, in place like the reference
        for (int i = 0; i < 4; ++i)
            if (zn.mat_live(i)) BCHK(h, apv_launch_add_rel_diag(n, q.Rq[i], i < 2 ? h->cfg.reg_bright : h->cfg.reg_dark, q.nrm + i, st));
    }
    return APV_OK;
}

// 6a: the spectra of the two input blocks as the ring holds them now
static int front_input_spectra(apv_handle* h, apv_bb* s, const BbHop& q, hipStream_t st) {
    std::string why;
    BCHK(h, apv_launch_analysis(1, s->N, 2, s->inblk, s->N, s->N, s->ring_off, 1, q.inspec, s->K, 1, st, &why));
    return APV_OK;
}

// stages 1-3 of a hop (and the input spectra of stage 6, which depend on the input ring as it stands now): everything in front
// of the joint diagonalisation.  t_stage: optional wall times of the stages (APV_BB_TIMING).
// st2 (optional, apv_bb_process_signal): the statistics of the hop run there, so that the next hop's K1 / WOLA chain on `st` does not
// wait for them -- the two halves of a hop are about equal at cfg1, ~40 us of small dependent launches each.  The rings order them:
// the statistics read the rings after this hop's append (ev_ring) and the next hop's append waits for them (ev_stat).
static int bb_front(apv_handle* h, apv_bb* s, const BbHop& q, double* t_stage, hipStream_t st, hipStream_t st2 = nullptr) {
    WallTimer timer;
    auto stage_done = [&]() {
        if (!t_stage) return;
        (void)hipStreamSynchronize(st);
        *t_stage++ = timer.lap();
    };
    int rc;
    if ((rc = front_history_and_rings(h, s, q, st)) != APV_OK) return rc;
    if ((rc = front_k1(h, s, st)) != APV_OK) return rc;
    stage_done();
    if ((rc = front_wola(h, s, st)) != APV_OK) return rc;
    // the finished hop, the head of the overlap buffers, goes to the statistics rings
    if (st2) BCHK(h, hipStreamWaitEvent(st, s->ev_stat, 0));          // the previous hop's statistics have read the rings
    BCHK(h, apv_launch_ring_append_f64(s->S, s->H, s->stat_off, s->ov_all, (long)s->N, s->stats_all, s->n_all, st));
    if (st2) {
        BCHK(h, hipEventRecord(s->ev_ring, st));
        BCHK(h, hipStreamWaitEvent(st2, s->ev_ring, 0));
    }
    stage_done();
    if ((rc = front_statistics(h, s, q, st2 ? st2 : st)) != APV_OK) return rc;
    if (st2) BCHK(h, hipEventRecord(s->ev_stat, st2));
    if ((rc = front_input_spectra(h, s, q, st)) != APV_OK) return rc;
    stage_done();
    return APV_OK;
}

// stages 5-6 of a hop: filter spectra, outputs, overlap-add.  The hop is emitted at d_out: channel-major [n_out][H], or with
// cfg.out_layout = 1 sample-major [n_out / L][H][L] (a group = one zone program and rank, or a target path: the (hop, loudspeaker)
// array the reference's caller receives, apvast.py:498-504) with `gstride` elements between groups (0: H L).  h_out (may be null):
// one contiguous hop copied to the host, queued on the handle's stream.
static int bb_back(apv_handle* h, apv_bb* s, const BbHop& q, double* d_out, long gstride, double* h_out, double* spec) {
    hipStream_t st = h->stream;
    const int N = s->N, H = s->H, K = s->K, L = s->L, J = s->J, V = s->V, n = s->n;
    const BbZones zn(s->zones);
    std::string why;
    // 5: filter spectra: channel (v, l) = taps w[v][l*J : (l+1)*J] zero-padded to N, no window; both zones' filters in one launch
    // when they lie one behind the other (they do: [zone][V][n] in the handle's arrays and in a group's slices)
    if (zn.nz == 2 && q.w[1] == q.w[0] + (size_t)V * n) {
        BCHK(h, apv_launch_analysis(1, N, 2 * V * L, q.w[0], J, J, 0, 0, s->fspec, K, 1, st, &why));
    } else {
        for (int z = 0; z < 2; ++z)
            if (zn.run[z])
                BCHK(h, apv_launch_analysis(1, N, V * L, q.w[z], J, J, 0, 0, s->fspec + (size_t)zn.slot(z) * V * L * K * 2, K, 1, st, &why));
    }
    // 6: outputs: the live zone programs' V L channels each, then the target paths A_t, B_t, in one launch
    ApplyJobsD aj{};
    int oc = 0;
    auto job = [&](int z, int channels) {
        aj.in[aj.n] = (const double2*)q.inspec + (size_t)z * K;
        aj.filt[aj.n] = (const double2*)s->fspec + (size_t)oc * K;
        aj.out[aj.n] = (double2*)spec + (size_t)oc * K;
        aj.first[aj.n++] = oc;
        oc += channels;
    };
    for (int z = 0; z < 2; ++z)
        if (zn.run[z]) job(z, V * L);
    for (int z = 0; z < 2; ++z) job(z, L);
    aj.first[aj.n] = oc;
    BCHK(h, apv_launch_apply_jobs_f64(K, aj, st));
    BCHK(h, apv_launch_synthesis(1, N, H, s->n_out, spec, K, 1, s->outov, d_out, st, &why, s->out_group, gstride));
    if (h_out) BCHK(h, hipMemcpyAsync(h_out, d_out, sizeof(double) * (size_t)s->n_out * H, hipMemcpyDeviceToHost, st));
    return APV_OK;
}

static int bb_group_size(const apv_handle* h, const apv_bb* s, int n_hops);

// ---- evaluation stage (apv_bb_set_evaluation) ---------------------------------------------------------------------------------------
// The emitted samples of n consecutive hops filtered through the responses to the validation microphones, on the handle's stream:
// ONE pressure launch over the n H samples (eval_pressure_kernel's bits depend on (Pv, L) and the data, not on the launch: a group
// of hops is a long hop with the history in front), the energies of each of the n hops into the record's slots slot0 .. slot0 + n - 1,
// and one launch that adds them to the totals in hop order and advances the histories.  d_out: the hops as bb_back emitted them --
// sample-major (cfg.out_layout = 1) group q's n H samples start at d_out + q gstride (0: H L) and are consecutive in time;
// channel-major [n_out][H], where only n = 1 is contiguous in time.     replaces: Matlab/main.m:64-76 with predictPressure.m:12-16
static int bb_evaluate(apv_handle* h, apv_bb* s, const double* d_out, size_t gstride, int n, int slot0) {
    hipStream_t st = h->stream;
    const int H = s->H, L = s->L, c = s->be_cur;
    const bool sample_major = s->out_group > 0;
    if (!sample_major && n != 1) return apv_fail(h, APV_ERR_ARG, "evaluation: channel-major hops are evaluated one at a time");
    if (n > s->be_p_hops || slot0 < 0 || slot0 + n > s->be_cap) return apv_fail(h, APV_ERR_STATE, "evaluation: buffers smaller than the launch");
    const size_t hop_stride = sample_major ? (gstride ? gstride : (size_t)H * L) : (size_t)L * H;
    const long sn = sample_major ? L : 1, sl = sample_major ? 1 : H;
    EvalPressureArgs a{};
    a.hist = s->be_hist[c]; a.hop = d_out;
    a.hist_stride = (size_t)(s->be_Pv - 1) * L; a.hop_stride = hop_stride;
    a.sn = sn; a.sl = sl;
    a.rv[0] = s->be_rv[0]; a.rv[1] = s->be_rv[1];
    a.map = s->be_map; a.p = s->be_p;
    a.n_sets = s->be_sets; a.Pv = s->be_Pv; a.H = n * H; a.L = L; a.Mv = s->be_Mv;
    std::string why;
    hipError_t e = apv_launch_eval_pressure(1, a, st, &why);
    if (e == hipSuccess) {
        BbEvalEnergyArgs en{};
        en.p = s->be_p; en.rec = s->be_rec; en.slot0 = slot0;
        en.Z = s->be_Z; en.E = s->be_E; en.H = H; en.Mv = s->be_Mv; en.n = n;
        e = apv_launch_bbeval_energies(en, st, &why);
    }
    if (e != hipSuccess) return apv_fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP, why.empty() ? hipGetErrorString(e) : why);
    BbEvalAdvanceArgs adv{};
    adv.rec = s->be_rec; adv.totals = s->be_tot;
    adv.old_hist = s->be_hist[c]; adv.new_hist = s->be_hist[c ^ 1];
    adv.hop = d_out; adv.hop_stride = hop_stride; adv.sn = sn; adv.sl = sl;
    adv.hist_src = s->be_hsrc;
    adv.slot0 = slot0; adv.Z = s->be_Z; adv.E = s->be_E; adv.H = H; adv.Mv = s->be_Mv; adv.n = n; adv.Pv = s->be_Pv; adv.L = L;
    adv.n_hist = s->be_nhist;
    BCHK(h, apv_launch_bbeval_advance(adv, st));
    if (s->be_Pv > 1) s->be_cur = c ^ 1;
    s->be_last = n;
    if (s->bs_on) {
        // the per-bin spectra of the same n hops: lines, transforms and |P|^2, in sub-launches of what the scratch holds
        BbSpecArgs sp{};
        sp.p = s->be_p; sp.p_set = (size_t)n * H * s->be_Mv;
        sp.line[0] = s->bs_line[0]; sp.line[1] = s->bs_line[1]; sp.cur = s->bs_cur; sp.len = s->bs_len;
        sp.spec = s->bs_spec; sp.totals = s->bs_tot;
        sp.N = s->N; sp.H = H; sp.Z = s->be_Z; sp.E = s->be_E; sp.Mv = s->be_Mv; sp.n = n; sp.per_launch = s->bs_hops;
        BbSpecDetectArgs det{};
        if (s->bd_on) {
            // and their detectability, inside every sub-launch: the record's slots are those of the energies
            if (slot0 + n > s->bd_cap) return apv_fail(h, APV_ERR_STATE, "evaluation detectability: record smaller than the launch");
            det.G2T = s->bd_G2T; det.quiet = s->bd_quiet; det.curves = s->bd_curves; det.part = s->bd_part;
            det.rec = s->bd_rec; det.totals = s->bd_tot; det.slot0 = slot0; det.C = s->bd_C;
            det.Cs = s->bd_Cs; det.Ca = s->bd_Ca; det.Leff = s->bd_Leff;
            sp.detect = &det;
        }
        e = apv_launch_bbspec_hops(&sp, st, &why);
        s->bs_cur = sp.cur; s->bs_len = sp.len;
        if (e != hipSuccess) return apv_fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP, why.empty() ? hipGetErrorString(e) : why);
        if (s->bd_on) s->bd_nrec = slot0 + n;
    }
    return APV_OK;
}

// curves and partial sums of the detectability for sub-launches of c hops: scratch, nothing of it outlives a sub-launch.  Called
// with nothing of the stage in flight.
static int bb_detect_scratch(apv_handle* h, apv_bb* s, int c) {
    const size_t cols = (size_t)s->be_Z * s->be_Mv, items = cols * 2 * s->be_E;
    double *curves = nullptr, *part = nullptr;
    if (s->own.device(&curves, sizeof(double) * (size_t)c * s->K * cols) != hipSuccess ||
        s->own.device(&part, sizeof(double) * (size_t)c * apv_eval_detect_chunks(s->N, s->be_Z, s->be_E, s->be_Mv) * items) != hipSuccess) {
        s->own.release(curves);
        return apv_fail(h, APV_ERR_HIP, "evaluation detectability: out of device memory for the curves of a sub-launch");
    }
    s->own.release(s->bd_curves);
    s->own.release(s->bd_part);
    s->bd_curves = curves; s->bd_part = part;
    return APV_OK;
}

// line buffers and scratch of the spectra for launches of `group` hops: sub-launches of as many hops as the scratch budget holds.
// The current line moves into the new buffers.  Called with nothing of the stage in flight.
static int bb_spec_reserve(apv_handle* h, apv_bb* s, int group) {
    const int c = std::min(group, apv_bbspec_hops_fit(s->N, s->be_Z, s->be_E, s->be_Mv));
    if (c <= s->bs_hops) return APV_OK;
    if (s->bd_on) {
        const int rc = bb_detect_scratch(h, s, c);           // first: on failure the spectra keep their sub-launch
        if (rc != APV_OK) return rc;
    }
    hipStream_t st = h->stream;
    const size_t ch = (size_t)s->be_sets * s->be_Mv, row = (size_t)s->N - s->H + (size_t)c * s->H;
    double* line[2] = {nullptr, nullptr};
    void* spec = nullptr;
    struct Guard {
        ApvOwned& own; double** line; void** spec; bool ok;
        ~Guard() { if (!ok) { own.release(line[0]); own.release(line[1]); own.release(*spec); } }
    } made{s->own, line, &spec, false};
    for (int b = 0; b < 2; ++b) BCHK(h, s->own.zeroed(&line[b], ch * row, sizeof(double), st));
    BCHK(h, s->own.device(&spec, sizeof(double) * 2 * (size_t)c * s->K * ch));
    if (s->bs_line[s->bs_cur])
        BCHK(h, hipMemcpyAsync(line[0], s->bs_line[s->bs_cur], sizeof(double) * ch * (size_t)s->bs_len, hipMemcpyDeviceToDevice, st));
    BCHK(h, hipStreamSynchronize(st));
    for (int b = 0; b < 2; ++b) s->own.release(s->bs_line[b]);
    s->own.release(s->bs_spec);
    s->bs_line[0] = line[0]; s->bs_line[1] = line[1]; s->bs_spec = spec;
    s->bs_cur = 0;
    s->bs_hops = c;
    made.ok = true;
    return APV_OK;
}

// the per-call record holds n_hops slots and the pressure buffer the launch of `group` hops; called before a call's first launch,
// with nothing of an earlier call in flight
static int bb_eval_reserve(apv_handle* h, apv_bb* s, int n_hops, int group) {
    const size_t slot = (size_t)s->be_Z * (3 * s->be_E + 1) * s->be_Mv;
    if (n_hops > s->be_cap) {
        s->own.release(s->be_rec);
        s->be_cap = 0;
        BCHK(h, s->own.zeroed(&s->be_rec, slot * n_hops, sizeof(double), h->stream));
        s->be_cap = n_hops;
    }
    if (group > s->be_p_hops) {
        s->own.release(s->be_p);
        s->be_p_hops = s->be_last = 0;
        BCHK(h, s->own.zeroed(&s->be_p, (size_t)s->be_sets * group * s->H * s->be_Mv, sizeof(double), h->stream));
        s->be_p_hops = group;
        BCHK(h, apv_eval_pressure_prepare(1, s->be_Pv, group * s->H, s->L));
    }
    s->be_nrec = 0;
    if (s->bd_on) {
        if (n_hops > s->bd_cap) {
            s->own.release(s->bd_rec);
            s->bd_cap = 0;
            BCHK(h, s->own.zeroed(&s->bd_rec, (size_t)s->be_Z * 2 * s->be_E * s->be_Mv * n_hops, sizeof(double), h->stream));
            s->bd_cap = n_hops;
        }
        s->bd_nrec = 0;
    }
    return s->bs_on ? bb_spec_reserve(h, s, group) : APV_OK;
}

static void bb_eval_free(apv_bb* s) {
    for (int z = 0; z < 2; ++z) {
        s->own.release(s->be_rv[z]);
        s->own.release(s->be_hist[z]);
    }
    s->own.release(s->be_map);
    s->own.release(s->be_hsrc);
    s->own.release(s->be_p);
    s->own.release(s->be_tot);
    s->own.release(s->be_rec);
    s->be_on = s->be_cap = s->be_nrec = s->be_p_hops = s->be_last = s->be_cur = 0;
}

static void bb_spec_free(apv_bb* s) {
    for (int b = 0; b < 2; ++b) s->own.release(s->bs_line[b]);
    s->own.release(s->bs_spec);
    s->own.release(s->bs_tot);
    s->bs_on = s->bs_hops = s->bs_cur = 0;
    s->bs_len = 0;
}

static void bb_detect_free(apv_bb* s) {
    s->own.release(s->bd_G2T);
    s->own.release(s->bd_quiet);
    s->own.release(s->bd_curves);
    s->own.release(s->bd_part);
    s->own.release(s->bd_tot);
    s->own.release(s->bd_rec);
    s->bd_on = s->bd_C = s->bd_cap = s->bd_nrec = 0;
}

// Evaluation stage of the broadband stream: see include/apvast_hip.h.
int apv_bb_set_evaluation(apv_handle* h, int32_t Pv, int32_t Mv, const double* h_rvA, const double* h_rvB, int32_t n_ranks,
                          const int32_t* ranks) {
    if (!h || !h->bb) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation: apv_bb_init has not been called");
    apv_bb* s = h->bb;
    if (s->be_on) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation: the stream has its evaluation stage already");
    if (!h_rvA || !h_rvB || !ranks) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation: null argument");
    if (Pv < 1 || Mv < 1) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation: Pv and Mv must be at least 1");
    if (!apv_eval_pressure_fits(Pv))
        return apv_fail(h, APV_ERR_ARG, "evaluation: one loudspeaker's window of Pv - 1 + 16 float64 samples does not fit 160 KB of LDS (Pv <= 20465)");
    if ((Mv + 15) / 16 > 65535) return apv_fail(h, APV_ERR_ARG, "evaluation: at most 16 x 65535 validation microphones");
    if (n_ranks < 1 || n_ranks > s->V) return apv_fail(h, APV_ERR_ARG, "evaluation: n_ranks must be within 1..the stream's ranks");
    const BbZones zn(s->zones);
    const int E = n_ranks, nz = zn.nz, V = s->V, L = s->L, H = s->H, nfilt = nz * V;
    const int sets = nz * (2 * E + 1), nhist = nz * (E + 1);
    // per zone program that runs, the pressure sets [bright of E ranks][dark of E ranks][target]; bright and target through the
    // responses of the program's own zone, dark through the other zone's (as apv_stream_init lays them out)
    std::vector<int32_t> map((size_t)4 * sets, 0), hsrc(nhist, 0);
    int zi = 0;
    for (int z = 0; z < 2; ++z) {
        if (!zn.run[z]) continue;
        for (int e = 0; e <= E; ++e) {
            int grp = nfilt + z;                             // e = E: the program's target output A_t / B_t
            if (e < E) {
                if (e && ranks[e] <= ranks[e - 1]) return apv_fail(h, APV_ERR_ARG, "evaluation: ranks must be strictly ascending");
                const auto it = std::find(s->rank_vals.begin(), s->rank_vals.end(), (int)ranks[e]);
                if (it == s->rank_vals.end()) return apv_fail(h, APV_ERR_ARG, "evaluation: a rank that the stream does not emit");
                grp = zi * V + (int)(it - s->rank_vals.begin());
            }
            const int hs = zi * (E + 1) + e;
            hsrc[hs] = grp;
            int32_t* mb = &map[(size_t)4 * (zi * (2 * E + 1) + (e < E ? e : 2 * E))];
            mb[0] = grp; mb[1] = hs; mb[2] = z;
            if (e < E) {
                int32_t* md = mb + 4 * E;
                md[0] = grp; md[1] = hs; md[2] = z ^ 1;
            }
        }
        ++zi;
    }
    std::string why;
    if (!apv_bbeval_sizes_ok(nz, E, H, Mv, 1, &why)) return apv_fail(h, APV_ERR_ARG, why);
    BCHK(h, hipSetDevice(h->device));
    BCHK(h, hipStreamSynchronize(h->stream));
    s->be_Pv = Pv; s->be_Mv = Mv; s->be_E = E; s->be_Z = nz; s->be_sets = sets; s->be_nhist = nhist;
    struct Guard { apv_bb* s; bool ok; ~Guard() { if (!ok) bb_eval_free(s); } } built{s, false};
    hipStream_t st = h->stream;
    const size_t bank = (size_t)Pv * L * Mv;
    for (int z = 0; z < 2; ++z) {
        BCHK(h, s->own.device(&s->be_rv[z], sizeof(double) * bank));
        BCHK(h, hipMemcpyAsync(s->be_rv[z], z ? h_rvB : h_rvA, sizeof(double) * bank, hipMemcpyHostToDevice, st));
    }
    BCHK(h, s->own.device(&s->be_map, sizeof(int32_t) * map.size()));
    BCHK(h, s->own.device(&s->be_hsrc, sizeof(int32_t) * hsrc.size()));
    BCHK(h, hipMemcpyAsync(s->be_map, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice, st));
    BCHK(h, hipMemcpyAsync(s->be_hsrc, hsrc.data(), sizeof(int32_t) * hsrc.size(), hipMemcpyHostToDevice, st));
    if (Pv > 1)
        for (int b = 0; b < 2; ++b) BCHK(h, s->own.zeroed(&s->be_hist[b], (size_t)nhist * (Pv - 1) * L, sizeof(double), st));
    BCHK(h, s->own.zeroed(&s->be_tot, (size_t)nz * (3 * E + 1) * Mv, sizeof(double), st));
    // the kernels a hop and the largest group of apv_bb_process_signal select, outside any timed path
    BCHK(h, apv_eval_pressure_prepare(1, Pv, H, L));
    BCHK(h, apv_eval_pressure_prepare(1, Pv, bb_group_size(h, s, INT_MAX) * H, L));
    const int rc = bb_eval_reserve(h, s, 1, 1);
    if (rc != APV_OK) return rc;
    BCHK(h, hipStreamSynchronize(st));                       // map, hsrc and the caller's responses may go
    s->be_on = 1;
    built.ok = true;
    return APV_OK;
}

// Per-bin spectra of the evaluation stage: see include/apvast_hip.h.
int apv_bb_set_evaluation_spectra(apv_handle* h, int32_t on) {
    if (!h || !h->bb) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_spectra: apv_bb_init has not been called");
    apv_bb* s = h->bb;
    if (!s->be_on) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_spectra: needs apv_bb_set_evaluation");
    if (s->bs_on) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_spectra: the stream keeps its evaluation spectra already");
    if (on != 1) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_spectra: on must be 1");
    std::string why;
    if (!apv_bbspec_size_ok(s->N, s->H, s->be_Z, s->be_E, s->be_Mv, &why)) return apv_fail(h, APV_ERR_ARG, why);
    BCHK(h, hipSetDevice(h->device));
    BCHK(h, hipStreamSynchronize(h->stream));
    struct Guard { apv_bb* s; bool ok; ~Guard() { if (!ok) bb_spec_free(s); } } built{s, false};
    BCHK(h, apv_stft_prepare(s->N, 1));                      // the float64 tables, outside any timed path
    BCHK(h, s->own.zeroed(&s->bs_tot, (size_t)s->be_Z * (3 * s->be_E + 1) * s->K * s->be_Mv, sizeof(double), h->stream));
    // lines for the launches the pressure buffer holds now; an empty line of N zeros per channel stands in front of the first hop
    s->bs_len = s->N;
    const int rc = bb_spec_reserve(h, s, std::max(s->be_p_hops, 1));
    if (rc != APV_OK) return rc;
    s->bs_on = 1;
    built.ok = true;
    return APV_OK;
}

// Perceptual detectability behind the per-bin spectra: see include/apvast_hip.h.
int apv_bb_set_evaluation_detectability(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff) {
    if (!h || !h->bb) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_detectability: apv_bb_init has not been called");
    apv_bb* s = h->bb;
    if (!s->bs_on) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_detectability: needs apv_bb_set_evaluation_spectra");
    if (s->bd_on) return apv_fail(h, APV_ERR_ARG, "apv_bb_set_evaluation_detectability: the stream keeps its detectabilities already");
    if (n_channels < 1 || n_channels > 512 || !h_G2) return apv_fail(h, APV_ERR_ARG, "evaluation detectability: a table of 1..512 channels");
    if (!std::isfinite(Cs) || !std::isfinite(Ca) || !std::isfinite(Leff) || !(Ca > 0.0))
        return apv_fail(h, APV_ERR_ARG, "evaluation detectability: Cs, Ca and Leff must be finite, Ca positive");
    const int K = s->K, Cn = n_channels;
    for (size_t i = 0; i < (size_t)K * Cn; ++i)
        if (!std::isfinite(h_G2[i])) return apv_fail(h, APV_ERR_ARG, "evaluation detectability: the table must be finite");
    std::string why;
    if (!apv_eval_detect_size_ok(s->N, s->be_Z, s->be_E, s->be_Mv, Cn, &why)) return apv_fail(h, APV_ERR_ARG, why);
    BCHK(h, hipSetDevice(h->device));
    BCHK(h, hipStreamSynchronize(h->stream));
    struct Guard { apv_bb* s; bool ok; ~Guard() { if (!ok) bb_detect_free(s); } } built{s, false};
    hipStream_t st = h->stream;
    std::vector<double> gt((size_t)Cn * K);                  // channel-major, as the curve kernel streams it
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < Cn; ++i) gt[(size_t)i * K + k] = h_G2[(size_t)k * Cn + i];
    s->bd_C = Cn; s->bd_Cs = Cs; s->bd_Ca = Ca; s->bd_Leff = Leff;
    BCHK(h, s->own.device(&s->bd_G2T, sizeof(double) * gt.size()));
    BCHK(h, hipMemcpyAsync(s->bd_G2T, gt.data(), sizeof(double) * gt.size(), hipMemcpyHostToDevice, st));
    BCHK(h, s->own.device(&s->bd_quiet, sizeof(double) * K));
    const size_t items = (size_t)s->be_Z * 2 * s->be_E * s->be_Mv;
    BCHK(h, s->own.zeroed(&s->bd_tot, 3 * items, sizeof(double), st));
    // the record as large as the energies', curves and partial sums for the sub-launches the scratch holds now
    const int cap = std::max(s->be_cap, 1);
    BCHK(h, s->own.zeroed(&s->bd_rec, items * cap, sizeof(double), st));
    s->bd_cap = cap;
    const int rc = bb_detect_scratch(h, s, std::max(s->bs_hops, 1));
    if (rc != APV_OK) return rc;
    BCHK(h, apv_launch_eval_detect_quiet(s->N, Cn, s->bd_G2T, Cs, Ca, Leff, s->bd_quiet, st));
    BCHK(h, hipStreamSynchronize(st));                       // gt may go
    s->bd_nrec = 0;
    s->bd_on = 1;
    built.ok = true;
    return APV_OK;
}

// "eval_totals" and both "eval_history" buffers to zero: the next hop's totals are its own energies; with the spectra on,
// "eval_spectra" and "eval_ring" too, with the detectability on "eval_detect"
int apv_bb_reset_evaluation(apv_handle* h) {
    if (!h || !h->bb || !h->bb->be_on) return apv_fail(h, APV_ERR_ARG, "apv_bb_reset_evaluation: no broadband stream with an evaluation stage");
    apv_bb* s = h->bb;
    BCHK(h, hipSetDevice(h->device));
    BCHK(h, hipMemsetAsync(s->be_tot, 0, sizeof(double) * (size_t)s->be_Z * (3 * s->be_E + 1) * s->be_Mv, h->stream));
    const size_t hb = sizeof(double) * (size_t)s->be_nhist * (s->be_Pv - 1) * s->L;
    for (int b = 0; b < 2 && hb > 0; ++b) BCHK(h, hipMemsetAsync(s->be_hist[b], 0, hb, h->stream));
    if (s->bs_on) {
        BCHK(h, hipMemsetAsync(s->bs_tot, 0, sizeof(double) * (size_t)s->be_Z * (3 * s->be_E + 1) * s->K * s->be_Mv, h->stream));
        BCHK(h, hipMemsetAsync(s->bs_line[s->bs_cur], 0, sizeof(double) * (size_t)s->be_sets * s->be_Mv * (size_t)s->bs_len, h->stream));
    }
    if (s->bd_on) BCHK(h, hipMemsetAsync(s->bd_tot, 0, sizeof(double) * (size_t)s->be_Z * 6 * s->be_E * s->be_Mv, h->stream));
    BCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

int apv_bb_process_block(apv_handle* h, const double* h_in_A, const double* h_in_B, double* h_out) {
    if (!h || !h_in_A || !h_in_B || !h_out) return apv_fail(h, APV_ERR_ARG, "null argument");
    apv_bb* s = h->bb;
    if (!s) return apv_fail(h, APV_ERR_ARG, "apv_bb_init has not been called");
    BCHK(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int H = s->H;
    const bool timing = bb_timing();
    double t_stage[5] = {0};
    std::memcpy(s->pin_in, h_in_A, sizeof(double) * H);
    std::memcpy(s->pin_in + H, h_in_B, sizeof(double) * H);
    BCHK(h, hipMemcpyAsync(s->xin, s->pin_in, sizeof(double) * 2 * H, hipMemcpyHostToDevice, st));
    const BbHop q = bb_own_hop(s);
    int rc = bb_front(h, s, q, timing ? t_stage : nullptr, st);
    if (rc != APV_OK) return rc;
    WallTimer timer;
    // 4: jdiag + filters; both zone programs in one batch when both run
    int32_t status[2] = {0, 0};
    if ((rc = bb_solve_own(h, s, true, status)) != APV_OK) return rc;
    s->full_valid = !h->gl_lead_done;
    if (timing) {
        (void)hipStreamSynchronize(st);
        t_stage[3] = timer.lap();
    }
    // a result array from apv_host_alloc receives the hop by DMA; any other goes through the handle's page-locked buffer and a copy
    const size_t out_bytes = sizeof(double) * (size_t)s->n_out * H;
    const bool direct = host_is_pinned(h_out, out_bytes, false);
    double* const dst = direct ? h_out : s->pin_out;
    rc = bb_back(h, s, q, s->out, 0, s->be_on ? nullptr : dst, s->spec);
    if (rc != APV_OK) return rc;
    if (s->be_on) {
        // the evaluation stage behind the synthesis, in front of the copy back
        s->be_nrec = 0;
        if ((rc = bb_evaluate(h, s, s->out, 0, 1, 0)) != APV_OK) return rc;
        s->be_nrec = 1;
        BCHK(h, hipMemcpyAsync(dst, s->out, out_bytes, hipMemcpyDeviceToHost, st));
    }
    BCHK(h, hipStreamSynchronize(st));
    BCHK(h, hipGetLastError());
    if (!direct) std::memcpy(h_out, s->pin_out, out_bytes);
    if (timing)
        fprintf(stderr, "[apv bb] fir %.3f  wola %.3f  stats %.3f  gevd %.3f  out %.3f ms\n", t_stage[0], t_stage[1],
                t_stage[2], t_stage[3], timer.lap());
    if (status[0] == 2 || status[1] == 2) {
        s->not_converged++;
        return apv_fail(h, APV_ERR_NO_CONVERGE, "eigen-iteration did not converge (Jacobi sweep cap reached); the outputs of this hop were written");
    }
    return APV_OK;
}

// ---- apv_bb_process_signal: n_hops consecutive hops in one call ------------------------------------------------------------------
// A hop's statistics depend on the input alone, never on an earlier hop's filters, so the joint diagonalisations of G consecutive
// hops are independent problems: the front stages of the G hops run one after the other (rings and overlap buffers are sequential
// state), ONE batched apv_gevd_large call solves their 2 G pairs -- a single n = 256 pair keeps 36 workgroups busy through ~180
// dependent launches, G pairs ride in the same launches -- and the output stages follow in order.  Sample for sample the result is
// that of n_hops calls of apv_bb_process_block up to the rounding of the eigen-iteration (a batch sweeps until its slowest member has
// converged).                                         replaces the hop loop of main.m:52-62 around apvast.py:153-165

// What one call needs.  Two buffer sets: the front stages of group g + 1 fill one while the solve of group g reads the other.
struct BbSignalCall {
    apv_handle* h;
    apv_bb* s;
    BbZones zn;
    int n_hops, G, n_groups;
    const double *in_A, *in_B;
    double* out;
    size_t z_xin, z_mat, z_vec, z_w, z_nrm, z_insp, z_out;      // doubles of one buffer set, for the CURRENT G
    // The caller's array: [n_out / L][n_hops H][L] with cfg.out_layout = 1 (every group's samples of the whole signal in a row: what
    // the class hands out without touching it), else [n_hops][n_out][H].  A group of hops is written on the device as the slice of
    // that array it is, and goes to the host in ONE copy: by DMA straight into the caller's array when that is page-locked
    // (apv_host_alloc: `direct`), else into the staging set, from where the host moves it while the device works on the next group.
    // (Before: one copy per hop into the pageable array -- which the runtime stages and waits for -- and the class transposed the
    // whole signal afterwards: at the reference's test parameters, 5.2 MB a hop, that was 2.9 of the 3.5 ms a hop took.)
    size_t ngrp, HL;       // rows of the caller's array (groups of channels; one when channel-major) and doubles of a hop in a row
    bool direct;
    hipStream_t fs, cs;    // front stream; copy stream (the handle's own where the outputs are small)
    std::vector<BbHop> hops[2];
    std::vector<int32_t> status;
    long bad_hops = 0;
    // The front stages of group g + 1 (~18 runtime calls a hop) are enqueued by a helper thread while the caller's solves group g:
    // the solve's passes block the host, and with the statistics on a stream of their own a group is bound by the host's enqueueing,
    // not by the device any more (0.6 ms of a group's 1.6 at cfg1).  Only the caller's thread writes the handle's message: the
    // helper's apv_fail calls write thr_err (apv_fail_redirect), an exception becomes APV_ERR_HIP there, and the caller's thread
    // reports either after the join.
    std::thread thr;
    int thr_rc = APV_OK;
    std::string thr_err;

    int set(int g) const { return g & 1; }
    int hop0(int g) const { return g * G; }
    int count(int g) const { return n_hops - g * G < G ? n_hops - g * G : G; }
    double* gout(int g) const { return s->g_out + set(g) * z_out; }
    double* nrm_dark(int g) const { return s->g_nrm + set(g) * z_nrm + (size_t)G * 4; }
};

// Hops per group: eight or sixteen, or as many as keep the group's matrices (two buffer sets here, the solver's workspace: ~19 arrays
// of n x n doubles per hop and zone) within 8 GB.  (Rounds 2-3 capped the group where the block-round launches of the batch
// reached ~3 workgroups per compute unit, which left n = 800 at one hop per group: but a round there is its pair-solve chain,
// not the chip -- tools/probes/large_batch_scaling.py: 7.5 / 4.9 / 4.1 ms per matrix at batch 2 / 4 / 8 -- and the whole
// signal went 21.2 -> 15.2 / 13.0 / 11.9 ms per hop with groups of 2 / 4 / 8, under the 16.7 ms a hop of audio lasts.)
static int bb_group_size(const apv_handle* h, const apv_bb* s, int n_hops) {
    const size_t per_hop_bytes = (size_t)19 * s->n * s->n * sizeof(double) * BbZones(s->zones).nz;
    // sixteen while the group stays within 1 GiB (cfg1: 0.78 / 0.68 / 0.61 / 0.62 / 0.61 ms per hop with 8 / 12 / 16 / 24 / 32 hops
    // a group), eight beyond (n = 800: 11.0 ms per hop with eight, 12.0 with sixteen: 3 GB of matrices no longer sit in the
    // Infinity Cache and the batch sweeps until its slowest member is done), fewer only to stay within 8 GiB
    // (round 4: with the leading-eigenpair solver a batch no longer sweeps until its slowest member is done, and sixteen hops a
    // group are the better choice at n = 800 too: 4.83 ms per hop against 4.98 with eight, profiles/r04/bb_group_sweep.txt)
    const bool lead = h->cfg.max_sweeps <= 0 && apv_gevd_lead_block(s->n, s->max_rank) > 0;
    int G;
    if (16 * per_hop_bytes <= ((size_t)(lead ? 8 : 1) << 30)) G = 16;
    else {
        G = (int)(((size_t)8 << 30) / per_hop_bytes);
        G = G < 1 ? 1 : (G > 8 ? 8 : G);
    }
    return G > n_hops ? n_hops : G;
}

// streams and events of the signal path, made once per stream state
static int bb_signal_streams(apv_handle* h, apv_bb* s, int G) {
    if (s->front) return APV_OK;
    BCHK(h, s->own.stream(&s->front, hipStreamNonBlocking));
    // a copy stream of its own only where a group's outputs are large enough for the next group's solve to notice the
    // transfer (84 MB at the reference's test parameters; 131 KB at cfg1: there the copy rides on the handle's stream --
    // every stream fewer is one fewer to share the runtime's few hardware queues with)
    if (sizeof(double) * (size_t)G * s->n_out * s->H >= ((size_t)4 << 20)) BCHK(h, s->own.stream(&s->copy, hipStreamNonBlocking));
    BCHK(h, s->own.stream(&s->front2, hipStreamNonBlocking));
    BCHK(h, s->own.event(&s->ev_ring, hipEventDisableTiming));
    BCHK(h, s->own.event(&s->ev_stat, hipEventDisableTiming));
    for (int i = 0; i < 2; ++i) {
        BCHK(h, s->own.event(&s->ev_front[i], hipEventDisableTiming));
        BCHK(h, s->own.event(&s->ev_back[i], hipEventDisableTiming));
        BCHK(h, s->own.event(&s->ev_out[i], hipEventDisableTiming));
    }
    return APV_OK;
}

// the set sizes for this call's G, and group buffers, staging, streams and events that hold them (a handle whose group buffers were
// sized for a larger G keeps them: the set offsets follow the CURRENT G)
static int bb_signal_prepare(BbSignalCall& c) {
    apv_handle* h = c.h;
    apv_bb* s = c.s;
    const size_t G = c.G, gz = G * c.zn.nz, nn = (size_t)s->n * s->n;
    c.n_groups = (c.n_hops + c.G - 1) / c.G;
    c.z_xin = G * 2 * s->H; c.z_mat = gz * nn; c.z_vec = gz * s->n; c.z_w = gz * s->V * s->n; c.z_nrm = G * 4 + gz;
    c.z_insp = G * 2 * s->K * 2; c.z_out = G * s->n_out * s->H;
    if (s->grp < c.G) {
        double** bufs[] = {&s->g_xin, &s->g_RA, &s->g_RB, &s->g_U, &s->g_lam, &s->g_r, &s->g_w, &s->g_nrm, &s->g_inspec, &s->g_out};
        for (double** b : bufs) s->own.release(*b);
        s->grp = 0;
        int rc;
        if ((rc = dalloc(h, &s->g_xin, 2 * c.z_xin))) return rc;
        if ((rc = dalloc(h, &s->g_RA, 2 * c.z_mat))) return rc;
        if ((rc = dalloc(h, &s->g_RB, 2 * c.z_mat))) return rc;
        if ((rc = dalloc(h, &s->g_U, c.z_mat))) return rc;                  // U, lam: written and read by the back half only
        if ((rc = dalloc(h, &s->g_lam, c.z_vec))) return rc;
        if ((rc = dalloc(h, &s->g_r, 2 * c.z_vec))) return rc;
        if ((rc = dalloc(h, &s->g_w, c.z_w))) return rc;
        if ((rc = dalloc(h, &s->g_nrm, 2 * c.z_nrm))) return rc;
        if ((rc = dalloc(h, &s->g_inspec, 2 * c.z_insp))) return rc;
        if ((rc = dalloc(h, &s->g_out, 2 * c.z_out))) return rc;
        s->own.release(s->g_pin_in);
        BCHK(h, s->own.pinned(&s->g_pin_in, sizeof(double) * 2 * c.z_xin));
        if (!s->spec_out && (rc = dalloc(h, &s->spec_out, (size_t)s->n_out * s->K * 2))) return rc;
        if ((rc = bb_signal_streams(h, s, c.G))) return rc;
        BCHK(h, hipStreamSynchronize(h->stream));            // the zero fills
        s->grp = c.G;
    }
    const int og = s->out_group;
    c.ngrp = og > 0 ? (size_t)s->n_out / og : 1;
    c.HL = (size_t)s->H * (og > 0 ? og : s->n_out);
    c.direct = host_is_pinned(c.out, sizeof(double) * (size_t)c.n_hops * s->n_out * s->H, true);
    if (!c.direct && s->g_pin_cap < c.z_out) {
        s->own.release(s->g_pin);
        s->g_pin_cap = 0;
        BCHK(h, s->own.pinned(&s->g_pin, sizeof(double) * 2 * c.z_out));
        s->g_pin_cap = c.z_out;
    }
    if (s->be_on) {
        const int rc = bb_eval_reserve(h, s, c.n_hops, s->out_group > 0 ? c.G : 1);
        if (rc != APV_OK) return rc;
        BCHK(h, hipStreamSynchronize(h->stream));            // the zero fills
    }
    c.fs = s->front;
    c.cs = s->copy ? s->copy : h->stream;
    c.status.assign(gz, 0);
    return APV_OK;
}

// where hop i of a group lives in buffer set `set`
static BbHop signal_hop(const BbSignalCall& c, int set, int i) {
    const apv_bb* s = c.s;
    const size_t n = s->n, nn = n * n;
    BbHop q{};
    q.xin = s->g_xin + set * c.z_xin + (size_t)i * 2 * s->H;
    for (int z = 0; z < 2; ++z) {
        if (!c.zn.run[z]) continue;
        const size_t slot = (size_t)i * c.zn.nz + c.zn.slot(z);
        q.Rq[z] = s->g_RA + set * c.z_mat + slot * nn;
        q.Rq[2 + z] = s->g_RB + set * c.z_mat + slot * nn;
        q.r[z] = s->g_r + set * c.z_vec + slot * n;
        q.w[z] = s->g_w + slot * s->V * n;
    }
    q.nrm = s->g_nrm + set * c.z_nrm + (size_t)i * 4;
    q.nrm_dark = s->g_nrm + set * c.z_nrm + (size_t)c.G * 4 + (size_t)i * c.zn.nz;
    q.inspec = s->g_inspec + set * c.z_insp + (size_t)i * 2 * s->K * 2;
    return q;
}

// the front stages of group g, all on the front stream (rings, histories and overlap buffers are sequential state); may run on
// the helper thread
static int signal_front(BbSignalCall& c, int g) {
    apv_handle* h = c.h;
    apv_bb* s = c.s;
    const int set = c.set(g), h0 = c.hop0(g), g_n = c.count(g), H = s->H;
    // (one copy per group from page-locked staging: two copies per hop from the caller's pageable arrays were 32 blocking calls)
    double* const pin = s->g_pin_in + set * c.z_xin;
    if (g >= 2) (void)hipEventSynchronize(s->ev_front[set]);        // group g - 2's copy out of this staging set has run
    for (int i = 0; i < g_n; ++i) {
        std::memcpy(pin + (size_t)i * 2 * H, c.in_A + (size_t)(h0 + i) * H, sizeof(double) * H);
        std::memcpy(pin + (size_t)i * 2 * H + H, c.in_B + (size_t)(h0 + i) * H, sizeof(double) * H);
    }
    BCHK(h, hipMemcpyAsync(s->g_xin + set * c.z_xin, pin, sizeof(double) * (size_t)g_n * 2 * H, hipMemcpyHostToDevice, c.fs));
    c.hops[set].assign(g_n, BbHop{});
    for (int i = 0; i < g_n; ++i) {
        c.hops[set][i] = signal_hop(c, set, i);
        // the statistics on a stream of their own, beside the next hop's K1 / WOLA chain
        const int rc = bb_front(h, s, c.hops[set][i], nullptr, c.fs, s->front2);
        if (rc != APV_OK) return rc;
    }
    BCHK(h, hipStreamWaitEvent(c.fs, s->ev_stat, 0));          // the last hop's statistics belong to the group
    BCHK(h, hipEventRecord(s->ev_front[set], c.fs));
    BCHK(h, hipGetLastError());                                // the launches of this thread
    return APV_OK;
}

// group g fills the other set, which the back half of group g - 2 has read (its event is on the handle's stream); enqueued by the
// helper thread
static int signal_start_front(BbSignalCall& c, int g) {
    if (g >= 2) BCHK(c.h, hipStreamWaitEvent(c.fs, c.s->ev_back[c.set(g)], 0));
    c.thr = std::thread([&c, g] {
        apv_fail_redirect(&c.thr_err);
        try {
            const hipError_t e = hipSetDevice(c.h->device);
            c.thr_rc = e != hipSuccess ? apv_fail(c.h, APV_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e))
                                       : signal_front(c, g);
        } catch (...) {                  // (host memory, most likely: no message is built here, that could throw again)
            c.thr_rc = APV_ERR_HIP;
            c.thr_err.clear();
        }
        apv_fail_redirect(nullptr);
    });
    return APV_OK;
}

static int signal_join_front(BbSignalCall& c) {
    if (!c.thr.joinable()) return APV_OK;
    c.thr.join();
    if (c.thr_rc == APV_OK) return APV_OK;
    return apv_fail(c.h, c.thr_rc, c.thr_err.empty() ? "exception while enqueueing the next group's front stages" : c.thr_err);
}

// ONE batched solve of the group's hops and zones
static int signal_solve(BbSignalCall& c, int g) {
    apv_bb* s = c.s;
    const int set = c.set(g);
    const int rc = bb_solve(c.h, s, s->g_RA + set * c.z_mat, s->g_RB + set * c.z_mat, c.nrm_dark(g), s->g_U, s->g_lam,
                            s->g_r + set * c.z_vec, s->g_w, c.count(g) * c.zn.nz, c.status.data());
    if (rc != APV_OK) return rc;
    if (g + 1 == c.n_groups) s->full_valid = !c.h->gl_lead_done;
    return APV_OK;
}

// the back stages of the group's hops, in order, into the group's slice of the caller's array on the device
static int signal_back(BbSignalCall& c, int g) {
    apv_bb* s = c.s;
    const int set = c.set(g), nz = c.zn.nz;
    if (g >= 2) BCHK(c.h, hipStreamWaitEvent(c.h->stream, s->ev_out[set], 0));          // group g - 2 has left this output set
    const long gstride = s->out_group > 0 ? (long)((size_t)c.G * c.HL) : 0;
    for (int i = 0; i < c.count(g); ++i) {
        const int rc = bb_back(c.h, s, c.hops[set][i], c.gout(g) + (size_t)i * c.HL, gstride, nullptr, s->spec_out);
        if (rc != APV_OK) return rc;
        bool bad = false;
        for (int z = 0; z < nz; ++z) bad = bad || c.status[(size_t)i * nz + z] == 2;
        c.bad_hops += bad;
    }
    if (s->be_on) {
        // the evaluation stage of the whole group: its samples are consecutive in time where the hops are emitted sample-major
        // (group g + 2's wait for ev_out[set] orders the reuse of this output set behind these launches too: the same stream)
        int rc = APV_OK;
        if (s->out_group > 0) rc = bb_evaluate(c.h, s, c.gout(g), (size_t)gstride, c.count(g), c.hop0(g));
        else
            for (int i = 0; i < c.count(g) && rc == APV_OK; ++i) rc = bb_evaluate(c.h, s, c.gout(g) + (size_t)i * c.HL, 0, 1, c.hop0(g) + i);
        if (rc != APV_OK) return rc;
        s->be_nrec = c.hop0(g) + c.count(g);
    }
    return APV_OK;
}

// the attributes of the handle are those of the last hop (apvast.py:368-403)
static int signal_leave_state(BbSignalCall& c, int g) {
    apv_handle* h = c.h;
    apv_bb* s = c.s;
    hipStream_t st = h->stream;
    const size_t n = s->n, nn = n * n, V = s->V;
    const int last = c.count(g) - 1;
    const BbHop& q = c.hops[c.set(g)][last];
    auto keep = [&](double* dst, const double* src, size_t count) {
        return hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToDevice, st);
    };
    for (int z = 0; z < 2; ++z) {
        if (!c.zn.run[z]) continue;
        const size_t slot = (size_t)last * c.zn.nz + c.zn.slot(z);
        BCHK(h, keep(s->R + z * nn, q.Rq[z], nn));
        BCHK(h, keep(s->R + (2 + z) * nn, q.Rq[2 + z], nn));
        BCHK(h, keep(s->r + z * n, q.r[z], n));
        BCHK(h, keep(s->w + z * V * n, q.w[z], V * n));
        BCHK(h, keep(s->U + z * nn, s->g_U + slot * nn, nn));
        BCHK(h, keep(s->lam + z * n, s->g_lam + slot * n, n));
    }
    BCHK(h, keep(s->nrm, q.nrm, 4));
    BCHK(h, keep(s->inspec, q.inspec, (size_t)2 * s->K * 2));
    return APV_OK;
}

// The group's set has been read for the last time (ev_back); its outputs go to the host: rows = groups of channels (one row when
// channel-major), count(g) hops wide; on the copy stream, so that the next group's solve does not wait for the transfer (84 MB =
// 1.7 ms of a group's 10 at the reference's test parameters)
static int signal_copy_out(BbSignalCall& c, int g) {
    apv_handle* h = c.h;
    apv_bb* s = c.s;
    const int set = c.set(g);
    const size_t width = (size_t)c.count(g) * c.HL, spitch = (size_t)c.G * c.HL, dpitch = (size_t)c.n_hops * c.HL;
    BCHK(h, hipEventRecord(s->ev_back[set], h->stream));
    BCHK(h, hipStreamWaitEvent(c.cs, s->ev_back[set], 0));
    if (c.direct) {
        BCHK(h, hipMemcpy2DAsync(c.out + (size_t)c.hop0(g) * c.HL, sizeof(double) * dpitch, c.gout(g), sizeof(double) * spitch,
                                 sizeof(double) * width, c.ngrp, hipMemcpyDeviceToHost, c.cs));
    } else {
        BCHK(h, hipMemcpyAsync(s->g_pin + set * s->g_pin_cap, c.gout(g), sizeof(double) * ((c.ngrp - 1) * spitch + width),
                               hipMemcpyDeviceToHost, c.cs));
    }
    BCHK(h, hipEventRecord(s->ev_out[set], c.cs));
    return APV_OK;
}

// group gg has arrived in its staging set: the host moves it into the caller's pageable array
static void signal_collect(BbSignalCall& c, int gg) {
    apv_bb* s = c.s;
    (void)hipEventSynchronize(s->ev_out[c.set(gg)]);
    copy_rows(c.out + (size_t)c.hop0(gg) * c.HL, (size_t)c.n_hops * c.HL, s->g_pin + c.set(gg) * s->g_pin_cap, (size_t)c.G * c.HL,
              (size_t)c.count(gg) * c.HL, c.ngrp);
}

// The groups in order.  Returns at the first status that is not OK with work possibly in flight: the caller drains.
static int signal_run(BbSignalCall& c) {
    apv_handle* h = c.h;
    apv_bb* s = c.s;
    hipStream_t st = h->stream;
    const bool timing = bb_timing();
    int rc;
    // per-hop calls before this one ran on the handle's stream: the front stream starts behind them
    BCHK(h, hipEventRecord(s->ev_back[0], st));
    BCHK(h, hipStreamWaitEvent(c.fs, s->ev_back[0], 0));
    if ((rc = signal_front(c, 0)) != APV_OK) return rc;
    for (int g = 0; g < c.n_groups; ++g) {
        const bool last = g + 1 == c.n_groups;
        WallTimer timer;
        double ms[6] = {0};
        if (!last && (rc = signal_start_front(c, g + 1)) != APV_OK) return rc;
        BCHK(h, hipStreamWaitEvent(st, s->ev_front[c.set(g)], 0));
        ms[0] = timer.lap();
        if (timing) {
            (void)hipStreamSynchronize(st);         // the group's front stages alone
            ms[1] = timer.lap();
        }
        if ((rc = signal_solve(c, g)) != APV_OK) return rc;
        ms[2] = timer.lap();
        if ((rc = signal_back(c, g)) != APV_OK) return rc;
        if (last && (rc = signal_leave_state(c, g)) != APV_OK) return rc;
        if ((rc = signal_copy_out(c, g)) != APV_OK) return rc;
        ms[3] = timer.lap();
        // the previous group has long arrived in its staging set: move it while the device works on this one
        if (!c.direct && g >= 1) signal_collect(c, g - 1);
        if (!c.direct && last) signal_collect(c, g);
        if ((rc = signal_join_front(c)) != APV_OK) return rc;
        if (timing) {
            ms[4] = timer.lap();
            (void)hipStreamSynchronize(st);
            ms[5] = timer.lap();
            fprintf(stderr, "[apv bb signal] group %d (%d hops): enqueue next front %.2f, wait for this front %.2f, solve %.2f, enqueue back %.2f, "
                    "collect %.2f, drain %.2f ms\n", g, c.count(g), ms[0], ms[1], ms[2], ms[3], ms[4], ms[5]);
        }
    }
    return APV_OK;
}

// joins the helper and waits for the (at most four) streams of the call: copies into the caller's array may be in flight
static hipError_t signal_drain(BbSignalCall& c) {
    if (c.thr.joinable()) c.thr.join();
    hipError_t first = hipSuccess;
    for (hipStream_t q : {c.fs, c.s->front2, c.h->stream, c.cs}) {
        const hipError_t e = hipStreamSynchronize(q);
        if (first == hipSuccess) first = e;
    }
    return first;
}

int apv_bb_process_signal(apv_handle* h, int32_t n_hops, const double* h_in_A, const double* h_in_B, double* h_out) {
    if (!h || !h_in_A || !h_in_B || !h_out) return apv_fail(h, APV_ERR_ARG, "null argument");
    apv_bb* s = h->bb;
    if (!s) return apv_fail(h, APV_ERR_ARG, "apv_bb_init has not been called");
    if (n_hops < 0) return apv_fail(h, APV_ERR_ARG, "n_hops must be >= 0");
    if (n_hops == 0) return APV_OK;
    BCHK(h, hipSetDevice(h->device));
    BbSignalCall c{h, s, BbZones(s->zones), n_hops, bb_group_size(h, s, n_hops), 0, h_in_A, h_in_B, h_out};
    int rc = bb_signal_prepare(c);
    if (rc != APV_OK) return rc;                   // nothing is in flight yet
    rc = signal_run(c);
    // the only place that drains, on every way out
    const hipError_t sync_err = signal_drain(c);
    if (rc != APV_OK) return rc;
    BCHK(h, sync_err);
    BCHK(h, hipGetLastError());
    if (c.bad_hops) {
        s->not_converged += c.bad_hops;
        return apv_fail(h, APV_ERR_NO_CONVERGE, "eigen-iteration did not converge (Jacobi sweep cap reached) in some hop; the outputs were written");
    }
    return APV_OK;
}

}  // extern "C"

long apv_bb_not_converged(const apv_handle* h) { return h->bb ? h->bb->not_converged : -1; }

extern "C" {

// Perceptual weighting for the broadband stream (see apv_stream_set_perceptual).      replaces apvast.py:313-324
int apv_bb_set_perceptual(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff,
                          int32_t normalisation) {
    if (!h || !h->bb) return apv_fail(h, APV_ERR_ARG, "apv_bb_init has not been called");
    apv_bb* s = h->bb;
    BCHK(h, hipSetDevice(h->device));
    BCHK(h, hipStreamSynchronize(h->stream));
    if (n_channels <= 0) {
        s->nch = 0;
        return APV_OK;
    }
    if (!h_G2 || n_channels > 512 || (normalisation != 0 && normalisation != 1)) return apv_fail(h, APV_ERR_ARG, "bad perceptual tables");
    const int K = s->K;
    s->own.release(s->G2);
    s->own.release(s->G2T);
    for (int z = 0; z < 2; ++z) s->own.release(s->Wgt[z]);
    std::vector<double> gt((size_t)n_channels * K);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < n_channels; ++i) gt[(size_t)i * K + k] = h_G2[(size_t)k * n_channels + i];
    int rc;
    if ((rc = dalloc(h, &s->G2, (size_t)K * n_channels))) return rc;
    if ((rc = dalloc(h, &s->G2T, (size_t)K * n_channels))) return rc;
    for (int z = 0; z < 2; ++z)
        if ((rc = dalloc(h, &s->Wgt[z], (size_t)K * s->M))) return rc;
    // behind the zero-fills of dalloc, on the same (the handle's) stream
    BCHK(h, hipMemcpyAsync(s->G2, h_G2, sizeof(double) * (size_t)K * n_channels, hipMemcpyHostToDevice, h->stream));
    BCHK(h, hipMemcpyAsync(s->G2T, gt.data(), sizeof(double) * gt.size(), hipMemcpyHostToDevice, h->stream));
    BCHK(h, hipStreamSynchronize(h->stream));               // gt goes out of scope
    s->nch = n_channels; s->Cs = Cs; s->Ca = Ca; s->Leff = Leff; s->norm_mode = normalisation;
    return APV_OK;
}

// New responses between two hops of the broadband stream; arguments and semantics as apv_stream_set_rirs (stream.hip).
//                                    replaces `ap.rir_A = ...` between two hops, read by lfilter(..., zi=state) at apvast.py:167-193
int apv_bb_set_rirs(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B, const double* h_trir_A,
                    const double* h_trir_B) {
    if (!h || !h->bb) return apv_fail(h, APV_ERR_ARG, "null argument / broadband stream not initialised");
    apv_bb* s = h->bb;
    if (rir_len != s->P) return apv_fail(h, APV_ERR_ARG, "rir_len must equal the stream's response length");
    BCHK(h, hipSetDevice(h->device));
    BCHK(h, hipStreamSynchronize(h->stream));
    const double* nw[4] = {h_rir_A, h_rir_B, h_trir_A, h_trir_B};
    FirLiveBanks b{};
    b.P = s->P; b.H = s->H; b.L = s->L; b.M = s->M; b.f64 = 1;
    for (int z = 0; z < 2; ++z) {
        b.rir[z] = s->rir[z];
        b.trir[z] = s->trir[z];
        b.hist_tail[z] = s->xhist[s->cur][z] + s->H;          // [P - 1 samples before the last hop | the last hop]: its last P - 1
    }
    const int rc = apv_live_update(h, s->live, b, nw, h->stream);
    if (rc != APV_OK) return rc;
    BCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

// state: "response<p>" [C][N], "target_response<z>" [M][N], "input_block" [2][N] (rings, logical order); "R<q>" [n][n]
// (AA, BB, AB, BA), "r" [2][n], "lambda" [2][n], "w" [2][V][n], "U<z>" [n][n] (columns = eigenvectors, descending),
// "stats<p>" [C][S], "target_stats<z>" [M][S] (rings, logical order); and what a bit-for-bit resume also needs:
// "input_history<g>" [P-1+H] (the reference's lfilter states, apvast.py:115-120, as the inputs they came from),
// "overlap<p>" [C][N], "target_overlap<z>" [M][N] (WOLA overlap buffers, apvast.py:132-137), "out_overlap" [n_out][N]
// (apvast.py:148-151), "filter_spectra" [n_out][K] c128 (apvast.py:394-403, 417-422)
static int bb_lookup(apv_handle* h, const char* name, double** d, size_t* count, int* rows, int* len, int* off) {
    apv_bb* s = h->bb;
    const std::string nm(name);
    *rows = 0;
    auto idx = [&](const char* pre, int maxv) -> int {
        const size_t pl = std::strlen(pre);
        if (nm.size() == pl + 1 && nm.compare(0, pl, pre) == 0 && nm[pl] >= '0' && nm[pl] < '0' + maxv) return nm[pl] - '0';
        return -1;
    };
    int q;
    if ((q = idx("response", 4)) >= 0) { *d = s->resp[q]; *count = (size_t)s->C * s->N; *rows = s->C; *len = s->N; *off = s->ring_off; return APV_OK; }
    if ((q = idx("target_response", 2)) >= 0) { *d = s->tresp[q]; *count = (size_t)s->M * s->N; *rows = s->M; *len = s->N; *off = s->ring_off; return APV_OK; }
    if ((q = idx("stats", 4)) >= 0) { *d = s->stats[q]; *count = (size_t)s->C * s->S; *rows = s->C; *len = s->S; *off = s->stat_off; return APV_OK; }
    if ((q = idx("target_stats", 2)) >= 0) { *d = s->tstats[q]; *count = (size_t)s->M * s->S; *rows = s->M; *len = s->S; *off = s->stat_off; return APV_OK; }
    if (nm == "input_block") { *d = s->inblk; *count = (size_t)2 * s->N; *rows = 2; *len = s->N; *off = s->ring_off; return APV_OK; }
    if ((q = idx("input_history", 2)) >= 0) { *d = s->xhist[s->cur][q]; *count = (size_t)s->P - 1 + s->H; return APV_OK; }
    if ((q = idx("overlap", 4)) >= 0) { *d = s->ov[q]; *count = (size_t)s->C * s->N; return APV_OK; }
    if ((q = idx("target_overlap", 2)) >= 0) { *d = s->tov[q]; *count = (size_t)s->M * s->N; return APV_OK; }
    if (nm == "out_overlap") { *d = s->outov; *count = (size_t)s->n_out * s->N; return APV_OK; }
    if (nm == "filter_spectra") { *d = s->fspec; *count = (size_t)s->n_out * s->K * 2; return APV_OK; }
    if ((q = idx("U", 2)) >= 0) { *d = s->U + (size_t)q * s->n * s->n; *count = (size_t)s->n * s->n; return APV_OK; }
    if ((q = idx("R", 4)) >= 0) { *d = s->R + (size_t)q * s->n * s->n; *count = (size_t)s->n * s->n; return APV_OK; }
    if (nm == "r") { *d = s->r; *count = (size_t)2 * s->n; return APV_OK; }
    if (nm == "lambda") { *d = s->lam; *count = (size_t)2 * s->n; return APV_OK; }
    if (nm == "w") { *d = s->w; *count = (size_t)2 * s->V * s->n; return APV_OK; }
    if (nm == "input_spectrum") { *d = s->inspec; *count = (size_t)2 * s->K * 2; return APV_OK; }
    if ((q = idx("weights", 2)) >= 0 && s->nch > 0) { *d = s->Wgt[q]; *count = (size_t)s->M * s->K; return APV_OK; }
    return apv_fail(h, APV_ERR_STATE, std::string("unknown broadband state name: ") + name);
}

// The names only a stream with the evaluation stage has, with the split of the subband stream's table (stream_state.hip):
// "eval_pressure" [Z][2 E + 1][H][Mv], the last hop's, and "eval_hops" [hops of the last call][Z][3 E + 1][Mv] are read-only;
// "eval_totals" [Z][3 E + 1][Mv] and "eval_history" [Z][E + 1][Pv - 1][L] (the buffer the next launch reads) can be set.  With the
// spectra on (apv_bb_set_evaluation_spectra) also "eval_spectra" [Z][3 E + 1][K][Mv] and "eval_ring" [Z (2 E + 1)][Mv][N], the
// last N samples of every channel of the current line; both can be set, a set ring becoming the current line.  With the
// detectability on (apv_bb_set_evaluation_detectability) also "eval_detect" [Z][6 E][Mv], which can be set, and "eval_detect_hops"
// [hops of the last call][Z][2 E][Mv], read-only.
struct BbEvalRef {
    double* d;
    size_t count;
    bool read_only, last_rows;      // last_rows: H rows of each set behind a launch of be_last hops
    bool line_end;                  // the last N samples of every row of the current line
};
static bool bb_eval_lookup(apv_bb* s, const char* name, BbEvalRef* r) {
    if (!s->be_on) return false;
    const size_t slot = (size_t)s->be_Z * (3 * s->be_E + 1) * s->be_Mv;
    const auto is = [&](const char* n) { return std::strcmp(name, n) == 0; };
    if (is("eval_pressure")) *r = BbEvalRef{s->be_p, (size_t)s->be_sets * s->H * s->be_Mv, true, true};
    else if (is("eval_hops")) *r = BbEvalRef{s->be_rec, slot * s->be_nrec, true, false};
    else if (is("eval_totals")) *r = BbEvalRef{s->be_tot, slot, false, false};
    else if (is("eval_history")) *r = BbEvalRef{s->be_hist[s->be_cur], (size_t)s->be_nhist * (s->be_Pv - 1) * s->L, false, false};
    else if (s->bs_on && is("eval_spectra")) *r = BbEvalRef{s->bs_tot, slot * s->K, false, false};
    else if (s->bs_on && is("eval_ring")) *r = BbEvalRef{s->bs_line[s->bs_cur], (size_t)s->be_sets * s->be_Mv * s->N, false, false, true};
    else if (s->bd_on && is("eval_detect")) *r = BbEvalRef{s->bd_tot, (size_t)s->be_Z * 6 * s->be_E * s->be_Mv, false, false};
    else if (s->bd_on && is("eval_detect_hops")) *r = BbEvalRef{s->bd_rec, (size_t)s->be_Z * 2 * s->be_E * s->be_Mv * s->bd_nrec, true, false};
    else return false;
    return true;
}

// The per-hop path solves for the eigenpairs the filters use (kernels_gevd_lead.hip).  lambda_* / U_* in full (apvast.py:380-387)
// are attributes somebody may read afterwards: the first read after such a hop runs the complete joint diagonalisation on
// the hop's matrices, which are still there (R is never modified by the solver).
static int bb_complete_eigenpairs(apv_handle* h) {
    apv_bb* s = h->bb;
    if (s->full_valid) return APV_OK;
    BCHK(h, hipSetDevice(h->device));
    int32_t status[2] = {0, 0};
    const int rc = bb_solve_own(h, s, false, status);
    if (rc != APV_OK) return rc;
    if (status[0] == 2 || status[1] == 2)
        return apv_fail(h, APV_ERR_NO_CONVERGE, "eigen-iteration did not converge (Jacobi sweep cap reached) while completing lambda / U");
    s->full_valid = 1;
    return APV_OK;
}

int apv_bb_get_state(apv_handle* h, const char* name, double* h_dst, size_t count) {
    if (!h || !h->bb || !name || !h_dst) return apv_fail(h, APV_ERR_ARG, "null argument / broadband stream not initialised");
    if (apv_live_index(name) >= 0) {
        apv_bb* s = h->bb;
        BCHK(h, hipSetDevice(h->device));
        return apv_live_state(h, s->live, apv_live_index(name), s->P, s->H, s->C, s->M, sizeof(double), h_dst, sizeof(double) * count,
                              true, h->stream);
    }
    BbEvalRef ev{};
    if (bb_eval_lookup(h->bb, name, &ev)) {
        apv_bb* s = h->bb;
        if (count != ev.count) return apv_fail(h, APV_ERR_STATE, "state size mismatch");
        if (ev.count == 0) return APV_OK;                    // "eval_history" with Pv = 1, "eval_hops" before the first hop
        BCHK(h, hipSetDevice(h->device));
        if (ev.last_rows) {
            const size_t hop = sizeof(double) * (size_t)s->H * s->be_Mv, last = s->be_last > 0 ? s->be_last : 1;
            BCHK(h, hipMemcpy2DAsync(h_dst, hop, ev.d + (last - 1) * (hop / sizeof(double)), last * hop, hop, s->be_sets,
                                     hipMemcpyDeviceToHost, h->stream));
        } else if (ev.line_end) {
            const size_t ring = sizeof(double) * (size_t)s->N;
            BCHK(h, hipMemcpy2DAsync(h_dst, ring, ev.d + (s->bs_len - s->N), sizeof(double) * (size_t)s->bs_len, ring,
                                     (size_t)s->be_sets * s->be_Mv, hipMemcpyDeviceToHost, h->stream));
        } else {
            BCHK(h, hipMemcpyAsync(h_dst, ev.d, sizeof(double) * ev.count, hipMemcpyDeviceToHost, h->stream));
        }
        BCHK(h, hipStreamSynchronize(h->stream));
        return APV_OK;
    }
    double* d; size_t need; int rows, len, off;
    int rc = bb_lookup(h, name, &d, &need, &rows, &len, &off);
    if (rc != APV_OK) return rc;
    if (!std::strcmp(name, "lambda") || !std::strcmp(name, "U0") || !std::strcmp(name, "U1")) {
        if ((rc = bb_complete_eigenpairs(h)) != APV_OK) return rc;
    }
    if (count != need) return apv_fail(h, APV_ERR_STATE, "state size mismatch");
    BCHK(h, hipSetDevice(h->device));
    if (rows == 0) {
        BCHK(h, hipMemcpyAsync(h_dst, d, sizeof(double) * need, hipMemcpyDeviceToHost, h->stream));
        BCHK(h, hipStreamSynchronize(h->stream));
        return APV_OK;
    }
    std::vector<double> tmp(need);
    BCHK(h, hipMemcpyAsync(tmp.data(), d, sizeof(double) * need, hipMemcpyDeviceToHost, h->stream));
    BCHK(h, hipStreamSynchronize(h->stream));
    ring_to_logical(h_dst, tmp.data(), rows, len, off, sizeof(double));
    return APV_OK;
}

int apv_bb_set_state(apv_handle* h, const char* name, const double* h_src, size_t count) {
    if (!h || !h->bb || !name || !h_src) return apv_fail(h, APV_ERR_ARG, "null argument / broadband stream not initialised");
    if (apv_live_index(name) >= 0) {
        apv_bb* s = h->bb;
        BCHK(h, hipSetDevice(h->device));
        BCHK(h, hipStreamSynchronize(h->stream));
        return apv_live_state(h, s->live, apv_live_index(name), s->P, s->H, s->C, s->M, sizeof(double), const_cast<double*>(h_src),
                              sizeof(double) * count, false, h->stream);
    }
    BbEvalRef ev{};
    if (bb_eval_lookup(h->bb, name, &ev)) {
        if (ev.read_only) return apv_fail(h, APV_ERR_STATE, std::string(name) + " is read-only");
        if (count != ev.count) return apv_fail(h, APV_ERR_STATE, "state size mismatch");
        if (ev.count == 0) return APV_OK;
        BCHK(h, hipSetDevice(h->device));
        BCHK(h, hipMemcpyAsync(ev.d, h_src, sizeof(double) * ev.count, hipMemcpyHostToDevice, h->stream));
        BCHK(h, hipStreamSynchronize(h->stream));
        if (ev.line_end) h->bb->bs_len = h->bb->N;           // the ring as given is the current line, N samples per channel
        return APV_OK;
    }
    double* d; size_t need; int rows, len, off;
    int rc = bb_lookup(h, name, &d, &need, &rows, &len, &off);
    if (rc != APV_OK) return rc;
    if (count != need) return apv_fail(h, APV_ERR_STATE, "state size mismatch");
    BCHK(h, hipSetDevice(h->device));
    if (rows == 0) {
        BCHK(h, hipMemcpyAsync(d, h_src, sizeof(double) * need, hipMemcpyHostToDevice, h->stream));
        BCHK(h, hipStreamSynchronize(h->stream));
        return APV_OK;
    }
    std::vector<double> tmp(need);
    ring_from_logical(tmp.data(), h_src, rows, len, off, sizeof(double));
    BCHK(h, hipMemcpyAsync(d, tmp.data(), sizeof(double) * need, hipMemcpyHostToDevice, h->stream));
    BCHK(h, hipStreamSynchronize(h->stream));               // tmp goes out of scope
    return APV_OK;
}

}  // extern "C"
