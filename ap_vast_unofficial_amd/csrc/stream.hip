// Streaming composition of the subband hot path: one call = one hop of both input signals.
//
//   apv_stream_init   : upload RIRs, allocate every buffer once      reference Python/apvast.py:97-151
//   apv_process_block : per hop                                       apvast.py:153-165
//       K1  RIR convolution of the hop to all control points          apvast.py:167-194
//       K2  sine-window analysis STFT of the response / target rings  apvast.py:197-203, 244-255
//       K5'-K10 per-bin correlate + jdiag + VAST filter, per zone     apvast.py:329-414 (subband form)
//       K3  output spectra = input spectrum x filter bank             apvast.py:445-452
//       K4  inverse STFT, window, overlap-add, emit first H samples   apvast.py:457-504
//
// Device layouts: control-point channel c = m*L + l (loudspeaker fastest), so a bin's control-point
// matrix X[k] = [M][L] is one contiguous slab of the bin-major spectra [K][M*L].
#include "stream_types.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

// the same inside the whole-signal path, whose callers add how far the call got (signal_bail)
#define SIGCHK(h, call) HIPCHK(h, call, "apv_process_signal")

// a launcher that failed: its own account of it where it gave one, else the runtime's
int launch_fail(apv_handle* h, hipError_t e, const std::string& why) {
    return apv_fail(h, APV_ERR_HIP, why.empty() ? hipGetErrorString(e) : why);
}

// `count` elements of `esz` bytes, zeroed, kept by the stream
template <typename T>
int dalloc(apv_handle* h, T** p, size_t count, size_t esz = sizeof(T)) {
    SCHK(h, h->st->own.zeroed(p, count, esz, h->stream));
    return APV_OK;
}

// front-end precision of a streaming handle: cfg.frontend = 0 follows compute_dtype, 1 forces float32, 2 float64
int frontend_f64(const apv_config& c) {
    if (c.frontend == 1) return 0;
    if (c.frontend == 2) return 1;
    return c.compute_dtype == APV_F64;
}

// Uploads go on the handle's stream, like the zero-fill of dalloc before them: that stream does not synchronise with the
// null stream, so a plain hipMemcpy could overtake the pending fill and be wiped by it.
template <typename T>
int upload_as(apv_handle* h, void* dst, const std::vector<double>& src) {
    std::vector<T> tmp(src.begin(), src.end());
    SCHK(h, hipMemcpyAsync(dst, tmp.data(), sizeof(T) * tmp.size(), hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));               // tmp goes out of scope
    return APV_OK;
}
int upload(apv_handle* h, int f64, void* dst, const std::vector<double>& src) {
    return f64 ? upload_as<double>(h, dst, src) : upload_as<float>(h, dst, src);
}

// bytes of one hop's result: [n_out][H] samples and, behind them, the [2][K] status words
inline size_t hop_out_bytes(const apv_stream* s) { return s->esz * (size_t)s->n_out * s->H; }
inline size_t hop_result_bytes(const apv_stream* s) { return hop_out_bytes(s) + sizeof(int32_t) * 2 * (size_t)s->K; }
inline const int32_t* hop_status_of(const apv_stream* s, const void* result) {
    return reinterpret_cast<const int32_t*>(static_cast<const char*>(result) + hop_out_bytes(s));
}

// path p: signal sig(p) through the RIRs of zone zone(p): AA, AB, BA, BB
inline int path_sig(int p) { return p >> 1; }
inline int path_zone(int p) { return p & 1; }

}  // namespace

// the captured launch sequences of the hops: captured again at the next hop of each phase
static void drop_hop_graphs(apv_stream* s) {
    for (hipGraphExec_t& e : s->execs) {
        if (e) (void)hipGraphExecDestroy(e);
        e = nullptr;
    }
}

void apv_stream_free(apv_handle* h) {
    apv_stream* s = h->st;
    if (!s) return;
    // the graphs and everything below may still be in flight on the handle's stream or the stream state's own (a re-init, an init
    // that failed half-way): wait for the device first, as the first hipFree of the buffers would
    (void)hipDeviceSynchronize();
    drop_hop_graphs(s);
    apv_live_free(s->live);
    delete s;
    h->st = nullptr;
}

// the spectra of one hop: set 0 is the handle's own (state arrays, apv_stream_get_statistics), set 1 exists once
// apv_process_signal has been called
struct HopSpectra {
    void* X[4];
    void* tspec[2];
    void* inspec;
};
static HopSpectra hop_spectra(const apv_stream* s, int set) {
    HopSpectra q;
    for (int p = 0; p < 4; ++p) q.X[p] = set ? s->X1[p] : s->X[p];
    for (int z = 0; z < 2; ++z) q.tspec[z] = set ? s->tspec1[z] : s->tspec[z];
    q.inspec = set ? s->inspec1 : s->inspec;
    return q;
}

// the hop forms R_B, R_D, r explicitly (window or forgetting) and the joint diagonalisation reads them: not the fused update
static inline bool explicit_stats(const apv_stream* s) { return s->win_T > 1 || s->fg_beta > 0.0; }

// Will the next hop's window hold fewer rows than the order of its pencils (fill phase of a stream with M < L, or T M < L
// throughout) AND would its solve go to kernels_gevd64.hip (order 64, float64 statistics)?  R_B and R_D then have rank below L,
// which that kernel does not solve (GevdParams::no_gevd64): such a hop takes the LDS kernel, and the un-captured launch sequence,
// so that the graphs stay those of the full window.  Every other order runs the same kernel whatever the rank, graphs included.
static bool win_low_rank(const apv_handle* h) {
    const apv_stream* s = h->st;
    const apv_config& c = h->cfg;
    if (s->win_T <= 1 || !s->win_c128 || !apv_gevd64_eligible(s->L, c.reg_mode, c.reg_bright, c.sweep_tol2)) return false;
    const long hops = s->win_fill_host + 1 < s->win_T ? s->win_fill_host + 1 : s->win_T;
    return hops * s->M < s->L;
}

// ---- job tables: each is filled in one place, for one hop (per-hop path, pipeline) and for a chunk of hops alike ----

// the zone programs that run, in zone order: z[0 .. nz)
struct LiveZones {
    int nz = 0, z[2];
    explicit LiveZones(const apv_stream* s) {
        for (int i = 0; i < 2; ++i)
            if (s->zones & (1 << i)) z[nz++] = i;
    }
};

// K1 by fast convolution, one launch for all six filter banks: the four response paths into the rows `resp`, the two target paths
// into `tresp` (the rings, or a chunk's linear buffers); `xspec` holds the spectra of the two input signals
struct K1Jobs {
    const void *jh[6], *jx[6];
    void* jr[6];
    int jc[6];
};
static K1Jobs k1_jobs(const apv_stream* s, void* const* resp, void* const* tresp, const void* xspec) {
    const size_t spec_bytes = ((size_t)s->fir_F / 2 + 1) * 2 * s->esz;      // one input spectrum
    K1Jobs j;
    for (int p = 0; p < 4; ++p) {
        j.jh[p] = s->rirspec[path_zone(p)]; j.jx[p] = (const char*)xspec + spec_bytes * path_sig(p);
        j.jr[p] = resp[p]; j.jc[p] = s->C;
    }
    for (int z = 0; z < 2; ++z) {
        j.jh[4 + z] = s->trirspec[z]; j.jx[4 + z] = (const char*)xspec + spec_bytes * z;
        j.jr[4 + z] = tresp[z]; j.jc[4 + z] = s->M;
    }
    return j;
}

// K2, every analysis transform in one launch: the live response paths, both targets, the two inputs, from the rows `resp`, `tresp`,
// `inblk` into the spectra set `q` (a chunk: into its first hop's set, hop i's jhop elements further on)
struct AnalysisJobs {
    const void* jx[7];
    void* jspec[7];
    int jch[7], nj = 0;
    long jsc[7], jsk[7], jhop[7];
};
static AnalysisJobs analysis_jobs(const apv_stream* s, void* const* resp, void* const* tresp, const void* inblk, const HopSpectra& q) {
    const bool runA = s->zones & 1, runB = s->zones & 2;
    const int K = s->K, M = s->M, C = s->C;
    AnalysisJobs j;
    int& nj = j.nj;
    for (int p = 0; p < 4; ++p) {
        const bool need = (p < 2) ? runA : runB;       // A->A, A->B feed zone program A; B->A, B->B feed B
        if (!need) continue;
        j.jx[nj] = resp[p]; j.jspec[nj] = q.X[p]; j.jch[nj] = C; j.jsc[nj] = s->xg; j.jsk[nj] = C;      // (xg, C): grouped when xg > 1
        j.jhop[nj] = (long)s->Kp * C; ++nj;
    }
    for (int z = 0; z < 2; ++z) {
        j.jx[nj] = tresp[z]; j.jspec[nj] = q.tspec[z]; j.jch[nj] = M; j.jsc[nj] = 1; j.jsk[nj] = M; j.jhop[nj] = (long)K * M; ++nj;
    }
    j.jx[nj] = inblk; j.jspec[nj] = q.inspec; j.jch[nj] = 2; j.jsc[nj] = K; j.jsk[nj] = 1; j.jhop[nj] = 2L * K; ++nj;
    return j;
}

// Perceptual weighting of the spectra set `q` (nothing where it is off): weights from the UNWEIGHTED target spectra
// (apvast.py:205), then spectra x weights (apvast.py:208-209, 258-262): A->A and B->A take zone A's curve, A->B and B->B zone B's
static int enqueue_weighting(apv_handle* h, const HopSpectra& q, hipStream_t st) {
    const apv_stream* s = h->st;
    if (s->nch <= 0) return APV_OK;
    const int K = s->K, L = s->L, M = s->M, C = s->C, f64 = s->f64;
    const bool runA = s->zones & 1, runB = s->zones & 2;
    for (int z = 0; z < 2; ++z)
        SCHK(h, apv_launch_perceptual_weights(f64, K, M, s->nch, q.tspec[z], s->G2, s->G2T, s->Cs, s->Ca, s->Leff, s->N,
                                              s->norm_mode, s->Wgt[z], st));
    for (int p = 0; p < 4; ++p) {
        const bool need = (p < 2) ? runA : runB;
        if (need) SCHK(h, apv_launch_scale_spectra(f64, K, C, L, q.X[p], s->Wgt[path_zone(p)], st));
    }
    for (int z = 0; z < 2; ++z) SCHK(h, apv_launch_scale_spectra(f64, K, M, 1, q.tspec[z], s->Wgt[z], st));
    return APV_OK;
}

// The fused solve (statistics and joint diagonalisation in one kernel) of both zone programs in ONE launch (blockIdx.y = zone;
// K = N/2+1 bins alone cannot fill the chip): spectra `q`, filters to wz / lamz, status words [2][K] at `status`.  The caller adds
// what belongs to its launch: yield_issue, no_gevd64, Lspill, and for a chunk n_hops and the hop_* strides.
static GevdParams fused_gevd_params(const apv_handle* h, const HopSpectra& q, void* const* wz, void* const* lamz, int32_t* status) {
    const apv_stream* s = h->st;
    const bool runA = s->zones & 1, runB = s->zones & 2;
    GevdParams p = apv_base_params(h);
    const int first = runA ? 0 : 1;
    p.x_c128 = s->f64;
    p.x_group = s->xg;
    p.XB = first ? q.X[3] : q.X[0];
    p.XD = first ? q.X[2] : q.X[1];
    p.d = q.tspec[first];
    p.w = wz[first];
    p.lam = lamz[first];
    p.status = status + (size_t)first * s->K;
    apv_span_first_zone(p, first);
    p.n_zones = (runA && runB) ? 2 : 1;
    if (p.n_zones == 2) {
        p.XB1 = q.X[3]; p.XD1 = q.X[2]; p.d1 = q.tspec[1];
        p.w1 = wz[1]; p.lam1 = lamz[1]; p.status1 = status + s->K;
    }
    return p;
}

// FIR synthesis: what its per-hop and per-chunk launches share.  Per live zone program the taps to fade from (`prev`) and to
// (`cur`), the signal it filters; the target paths (pure delays); the layout of the result.  The caller sets the input side
// (xhist, xhop), `out` and, for a chunk, n_hops and the hop_* strides.
static FirSynthArgs fir_synth_args(const apv_stream* s, void* const* prev, void* const* cur) {
    FirSynthArgs a{};
    const LiveZones lz(s);
    for (int i = 0; i < lz.nz; ++i) { a.prev[i] = prev[lz.z[i]]; a.cur[i] = cur[lz.z[i]]; a.sig[i] = lz.z[i]; }
    a.nz = lz.nz; a.nV = s->nV; a.L = s->L; a.J = s->taps; a.H = s->H;
    a.n_tgt = 2; a.ref = s->fs_ref; a.delay = s->fs_delay;
    a.sn = s->out_group > 0 ? s->L : 1;
    a.sl = s->out_group > 0 ? 1 : s->H;
    return a;
}

// Front half of a hop on stream `st`: pinned hop `pin_src` [2][H] -> input histories, response rings (K1), analysis
// spectra of set `set` (K2, perceptual weighting).  Advances (ring_off, cur) on the host.  Pure enqueue: also used
// under stream capture.
// `set_free` (whole-signal path): event to wait for before the first kernel that writes the spectra set.
static int enqueue_front(apv_handle* h, hipStream_t st, int set, const void* pin_src, hipEvent_t set_free = nullptr) {
    apv_stream* s = h->st;
    const HopSpectra q = hop_spectra(s, set);
    const int N = s->N, H = s->H, M = s->M, C = s->C, P = s->P, f64 = s->f64;
    // hop -> device, input history and input-block rings
    // the hop [A | B] is read by the input-update kernel straight from the pinned host staging (16 KB over PCIe inside a kernel
    // that has nothing else to do) instead of through a copy node of its own
    const int nxt = s->cur ^ 1;
    // all rings advance by one hop: logical sample n now lives H further on
    s->ring_off = (s->ring_off + H) % N;
    const void* oh[2] = {s->xhist[s->cur][0], s->xhist[s->cur][1]};
    void* nh[2] = {s->xhist[nxt][0], s->xhist[nxt][1]};
    // (the histories keep s->keep samples in front of the hop: P - 1, more when K1 is partitioned)
    SCHK(h, apv_launch_input_update(f64, s->keep + 1, H, s->pad, N, s->ring_off, oh, nh, pin_src, s->inblk, st));   // histories + input-block rings
    s->cur = nxt;
    // K1: RIR convolution into the response rings (one MFMA launch for all six filter banks)
    if (s->fir_F > 0) {
        if (s->fir_np > 1)
            SCHK(h, apv_launch_fir_input_spectra_parts(f64, s->fir_F, s->fir_np, s->xhist[s->cur][0], s->xhist[s->cur][1], s->xspec, st));
        else
            SCHK(h, apv_launch_fir_input_spectra(f64, s->fir_F, s->xhist[s->cur][0], s->xhist[s->cur][1], P - 1 + H, s->xspec, st));
        const K1Jobs j = k1_jobs(s, s->resp, s->tresp, s->xspec);
        SCHK(h, apv_launch_fir_fft_jobs(f64, s->fir_F, 6, j.jh, j.jx, j.jr, j.jc, P, H, N, s->ring_off, st, s->fir_np));
    } else if (f64) {
        FirJobsD jobs{};
        for (int p = 0; p < 4; ++p) {
            jobs.rir[p] = (const double*)s->rir[path_zone(p)]; jobs.xh[p] = (const double*)s->xhist[s->cur][path_sig(p)];
            jobs.resp[p] = (double*)s->resp[p]; jobs.C[p] = C;
        }
        for (int z = 0; z < 2; ++z) {
            jobs.rir[4 + z] = (const double*)s->trir[z]; jobs.xh[4 + z] = (const double*)s->xhist[s->cur][z];
            jobs.resp[4 + z] = (double*)s->tresp[z]; jobs.C[4 + z] = M;
        }
        SCHK(h, apv_launch_fir_jobs_f64(jobs, 6, P, H, N, s->ring_off, st));
    } else {
        FirJobs jobs;
        jobs.n = 6;
        for (int p = 0; p < 4; ++p)
            jobs.j[p] = FirJob{(const float*)s->rir[path_zone(p)], (const float*)s->xhist[s->cur][path_sig(p)], (float*)s->resp[p], C};
        for (int z = 0; z < 2; ++z)
            jobs.j[4 + z] = FirJob{(const float*)s->trir[z], (const float*)s->xhist[s->cur][z], (float*)s->tresp[z], M};
        SCHK(h, apv_launch_fir_jobs(jobs, P, H, N, s->ring_off, st));
    }
    if (s->live.hops_left > 0) {
        // responses replaced within the last P - 1 samples: the samples before the update still ring out through the old ones
        void* dst[6] = {s->resp[0], s->resp[1], s->resp[2], s->resp[3], s->tresp[0], s->tresp[1]};
        int rc = apv_live_apply(h, s->live, P, C, M, f64, dst, H, H, N, N - H + s->ring_off, N, st);
        if (rc != APV_OK) return rc;
        apv_live_advance(s->live, 1);
    }
    // K2: analysis, bin-major output
    if (set_free) SCHK(h, hipStreamWaitEvent(st, set_free, 0));       // histories, rings and K1 above did not need the set
    const AnalysisJobs j = analysis_jobs(s, s->resp, s->tresp, s->inblk, q);
    std::string why;
    hipError_t e = apv_launch_stft_analysis_jobs(f64, N, j.nj, j.jx, j.jch, j.jspec, j.jsc, j.jsk, s->ring_off, st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    return enqueue_weighting(h, q, st);
}

// Evaluation stage of a hop on stream `st`, behind the synthesis that wrote the result buffer `obuf` and in front of its copy back:
// the pressures of every set in one launch, then the energies, the record, the totals and the histories in a second.  After
// enqueue_front: the histories alternate with s->cur, and so do the two slot counters.  With the per-bin spectra on, three more
// launches behind them (kernels_evalspec.hip): they read s->ring_off as enqueue_front left it, like K1 and the analysis, so the
// period of the captured graphs is unchanged.
static int enqueue_eval(apv_handle* h, hipStream_t st, const void* obuf) {
    apv_stream* s = h->st;
    const int c = s->cur, H = s->H, L = s->L;
    EvalPressureArgs a{};
    a.hist = s->ev_hist[c ^ 1]; a.hop = obuf;
    a.hist_stride = (size_t)(s->ev_Pv - 1) * L; a.hop_stride = (size_t)H * L;
    a.sn = s->out_group > 0 ? L : 1;
    a.sl = s->out_group > 0 ? 1 : H;
    a.rv[0] = s->ev_rv[0]; a.rv[1] = s->ev_rv[1];
    a.map = s->ev_map; a.p = s->ev_p;
    a.n_sets = s->ev_sets; a.Pv = s->ev_Pv; a.H = H; a.L = L; a.Mv = s->ev_Mv;
    std::string why;
    hipError_t e = apv_launch_eval_pressure(s->f64, a, st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    EvalAdvanceArgs adv{};
    adv.p = s->ev_p; adv.totals = s->ev_tot; adv.ctl = s->ev_ctl; adv.par = c;
    adv.old_hist = s->ev_hist[c ^ 1]; adv.new_hist = s->ev_hist[c];
    adv.hop = obuf; adv.hop_stride = a.hop_stride; adv.sn = a.sn; adv.sl = a.sl;
    adv.hist_src = s->ev_hsrc;
    adv.Z = s->ev_Z; adv.E = s->ev_E; adv.H = H; adv.Mv = s->ev_Mv; adv.Pv = s->ev_Pv; adv.L = L; adv.n_hist = s->ev_nhist;
    SCHK(h, apv_launch_eval_advance(s->f64, adv, st));
    if (s->es_on) {
        EvalSpectraArgs sp{};
        sp.p = s->ev_p; sp.ring = s->es_ring; sp.spec = s->es_spec; sp.totals = s->es_tot;
        sp.ring_off = s->ring_off; sp.N = s->N; sp.H = H; sp.Z = s->ev_Z; sp.E = s->ev_E; sp.Mv = s->ev_Mv;
        e = apv_launch_eval_spectra(sp, st, &why);
        if (e != hipSuccess) return launch_fail(h, e, why);
    }
    if (s->ed_on) {
        // three more behind them, on the scratch the transform just filled: nothing here has a period (the record's slot is a device word)
        EvalDetectArgs d{};
        d.spec = s->es_spec; d.G2T = s->ed_G2T; d.quiet = s->ed_quiet; d.curves = s->ed_curves; d.part = s->ed_part;
        d.hop = nullptr; d.ctl = s->ed_ctl; d.totals = s->ed_tot;
        d.N = s->N; d.Z = s->ev_Z; d.E = s->ev_E; d.Mv = s->ev_Mv; d.C = s->ed_C;
        d.Cs = s->ed_Cs; d.Ca = s->ed_Ca; d.Leff = s->ed_Leff;
        e = apv_launch_eval_detect(d, st, &why);
        if (e != hipSuccess) return launch_fail(h, e, why);
    }
    return APV_OK;
}

// Start of a call of n_hops hops on an evaluated stream: the per-call record holds at least n_hops slots (grow-only), and the slot
// counter the call's first hop reads -- that of the parity enqueue_front will flip to -- is zero.
static int eval_begin_call(apv_handle* h, int n_hops) {
    apv_stream* s = h->st;
    hipStream_t st = h->stream;
    if (n_hops > s->ev_cap) {
        const size_t slot = sizeof(double) * (size_t)s->ev_Z * (3 * s->ev_E + 1) * s->ev_Mv;
        SCHK(h, hipStreamSynchronize(st));
        double* rec = nullptr;
        SCHK(h, s->own.device(&rec, slot * n_hops));
        s->own.release(s->ev_rec);
        s->ev_rec = rec;
        s->ev_cap = n_hops;
        const unsigned long long words[2] = {(unsigned long long)reinterpret_cast<uintptr_t>(rec), (unsigned long long)n_hops};
        SCHK(h, hipMemcpyAsync(s->ev_ctl, words, sizeof(words), hipMemcpyHostToDevice, st));
        SCHK(h, hipStreamSynchronize(st));                   // words goes out of scope
    }
    SCHK(h, hipMemsetAsync(s->ev_ctl + 2 + (s->cur ^ 1), 0, sizeof(unsigned long long), st));
    if (s->ed_on) {
        if (n_hops > s->ed_cap) {
            const size_t slot = sizeof(double) * (size_t)s->ev_Z * 2 * s->ev_E * s->ev_Mv;
            SCHK(h, hipStreamSynchronize(st));
            double* rec = nullptr;
            SCHK(h, s->own.device(&rec, slot * n_hops));
            s->own.release(s->ed_rec);
            s->ed_rec = rec;
            s->ed_cap = n_hops;
            const unsigned long long words[2] = {(unsigned long long)reinterpret_cast<uintptr_t>(rec), (unsigned long long)n_hops};
            SCHK(h, hipMemcpyAsync(s->ed_ctl, words, sizeof(words), hipMemcpyHostToDevice, st));
            SCHK(h, hipStreamSynchronize(st));               // words goes out of scope
        }
        SCHK(h, hipMemsetAsync(s->ed_ctl + 2, 0, sizeof(unsigned long long), st));
    }
    s->ev_nrec = 0;
    return APV_OK;
}

// Where the back half of a hop puts its results and how it is scheduled: the result buffer (samples, then status words) and the
// output spectra; for the whole-signal path an event to record once the spectra set has been read for the last time (after K3),
// and a stream of its own for synthesis and copy back, which start at that event.  The copy back goes to the pinned `pin_dst` of
// the stages; none where that is null (chunked whole-signal path: one copy per chunk, by the caller).
struct BackSchedule {
    char* result;
    char* ospec;
    int yield_issue = 0;      // GevdParams::yield_issue
    hipEvent_t spectra_free = nullptr;
    hipStream_t tail_stream = nullptr;
    hipEvent_t copied = nullptr;
    void* lspill = nullptr;   // GevdParams::Lspill of this launch (nullptr: the handle's d_Lspill)
    bool span_quiet = false;  // the launch does not write the span's outputs, nor the validation span's, nor the effort limit's
                              // (hops that run side by side on several back streams)
    BackSchedule(void* result_, void* ospec_) : result((char*)result_), ospec((char*)ospec_) {}
};

// ---- the stages of the back half of a hop.  enqueue_back runs them in order; the chunked whole-signal path, which makes some of
// them one launch per chunk, calls the others directly ----

// Per-bin filters (K5'-K10) of both zone programs from the spectra `q`, on `st`: filters to wz / lamz, status words behind the
// samples of the hop's result buffer.
// per-bin update per zone program: A: bright A->A, dark A->B, target A;  B: bright B->B, dark B->A, target B
static int back_solve(apv_handle* h, hipStream_t st, const HopSpectra& q, void* const* wz, void* const* lamz, const BackSchedule& sch) {
    apv_stream* s = h->st;
    auto hush = [&](GevdParams& p) {
        if (sch.span_quiet)
            for (SpanZone& z : p.span.z) { z.rank = nullptr; z.contrast = nullptr; }
    };
    int32_t* const status = reinterpret_cast<int32_t*>(sch.result + hop_out_bytes(s));
    const int K = s->K, L = s->L, f64 = s->f64;
    std::string why;
    if (explicit_stats(s)) {
        // statistics over the last win_T hops: this hop's Gram matrices into the ring and the window sums in one launch for both
        // zone programs (forgetting: beta x accumulator + Gram matrices, likewise one launch), then the joint diagonalisation from
        // explicit R_B, R_D, r (the launch apv_gevd_vast_dev makes), per zone
        const void *xb[2], *xd[2], *dd[2];
        void *ring[2], *RB[2], *RD[2], *rr[2];
        const LiveZones lz(s);
        const int nz = lz.nz;
        for (int i = 0; i < nz; ++i) {
            const int z = lz.z[i];
            xb[i] = z ? q.X[3] : q.X[0]; xd[i] = z ? q.X[2] : q.X[1]; dd[i] = q.tspec[z];
            ring[i] = s->win_ring[z]; RB[i] = s->win_RB[z]; RD[i] = s->win_RD[z]; rr[i] = s->win_r[z];
        }
        if (s->win_tm.ev[0]) SCHK(h, hipEventRecord(s->win_tm.ev[0], st));
        if (s->fg_beta > 0.0) SCHK(h, apv_launch_statforget(f64, s->win_c128, K, s->M, L, s->fg_beta, nz, xb, xd, dd, ring, RB, RD, rr, st));
        else SCHK(h, apv_launch_statwin(f64, s->win_c128, K, s->M, L, s->win_T, nz, xb, xd, dd, ring, RB, RD, rr, s->win_ctr, st));
        if (s->win_tm.ev[1]) SCHK(h, hipEventRecord(s->win_tm.ev[1], st));
        for (int i = 0; i < nz; ++i) {
            const int z = lz.z[i];
            GevdParams p = apv_base_params(h);
            p.RB = s->win_RB[z]; p.RD = s->win_RD[z]; p.r = s->win_r[z];
            p.w = wz[z]; p.lam = lamz[z]; p.status = status + (size_t)z * K;
            apv_span_first_zone(p, z);
            p.n_zones = 1;
            p.no_gevd64 = s->fg_beta > 0.0 ? s->fg_no_gevd64 : win_low_rank(h);
            if (sch.lspill) p.Lspill = sch.lspill;
            hush(p);
            hipError_t e = apv_launch_gevd(p, s->win_c128 ? APV_F64 : APV_F32, false, st, &why, h->rank_list.data());
            if (e != hipSuccess) return launch_fail(h, e, why);
        }
        return APV_OK;
    }
    GevdParams p = fused_gevd_params(h, q, wz, lamz, status);
    p.yield_issue = sch.yield_issue;
    // one block of fewer than L rows: win_low_rank's route at T = 1, on every hop (float64 arithmetic only, as in apv_update_dev)
    p.no_gevd64 = s->M < L && h->cfg.compute_dtype == APV_F64;
    if (sch.lspill) p.Lspill = sch.lspill;
    hush(p);
    hipError_t e = apv_launch_gevd(p, h->cfg.compute_dtype, true, st, &why, h->rank_list.data());
    if (e != hipSuccess) return launch_fail(h, e, why);
    return APV_OK;
}

// The hop's filters `wz` projected onto J-tap responses, in place, both zone programs in one launch (nothing in an unconstrained
// stream): K3, the attributes and the states read the projected filters; the taps go to wtaps.
static int back_constrain(apv_handle* h, hipStream_t st, void* const* wz) {
    apv_stream* s = h->st;
    if (s->taps <= 0) return APV_OK;
    void *cw[2], *ct[2];
    const LiveZones lz(s);
    for (int i = 0; i < lz.nz; ++i) { cw[i] = wz[lz.z[i]]; ct[i] = s->wtaps[lz.z[i]]; }
    std::string why;
    if (s->cf_tm.ev[0]) SCHK(h, hipEventRecord(s->cf_tm.ev[0], st));
    hipError_t e = apv_launch_constrain_filters(h->cfg.out_c128, s->N, s->taps, s->nV, s->L, lz.nz, cw, ct, st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    if (s->cf_tm.ev[1]) SCHK(h, hipEventRecord(s->cf_tm.ev[1], st));
    return APV_OK;
}

// The array-effort limit on n_hops filter sets, w[z] + i hop_w (elements) of the zone programs that run: one launch on `st`.  The
// outputs of the handle (apv_get_effort) are written by hop emit_hop of the launch (EFFORT_EMIT_NONE: by none).
static int effort_launch(apv_handle* h, hipStream_t st, void* const* w, int n_hops, size_t hop_w, int emit_hop) {
    const apv_stream* s = h->st;
    const apv_handle::Effort& ef = h->effort;
    const size_t K = s->K, nV = s->nV;
    EffortArgs a;
    const LiveZones lz(s);
    a.zones = lz.nz;
    for (int i = 0; i < lz.nz; ++i) {
        const size_t z = lz.z[i];
        a.w[i] = w[z];
        a.limit[i] = ef.d_limit + z * K;
        a.effort[i] = ef.d_effort + z * K * nV;
        a.src[i] = ef.d_src + z * K;
        a.gain[i] = ef.d_gain + z * K;
    }
    a.n_hops = n_hops;
    a.hop_w = hop_w;
    a.emit_hop = emit_hop;
    std::string why;
    hipError_t e = apv_launch_limit_effort(h->cfg.out_c128, s->K, s->nV, s->L, a, st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    return APV_OK;
}

// The hop's filters `wz` held to the per-bin effort limit, in place, both zone programs in one launch (nothing in a stream without
// a limit): the projection, K3, the attributes and the states read the limited filters.
static int back_limit_effort(apv_handle* h, hipStream_t st, void* const* wz, const BackSchedule& sch) {
    if (!h->effort.on) return APV_OK;
    return effort_launch(h, st, wz, 1, 0, sch.span_quiet ? EFFORT_EMIT_NONE : 0);
}

// The hop's filters `wz` put to the choice by validation contrast, in place, both zone programs in one launch (nothing in a stream
// without apv_stream_set_validation_span): program A's bright bank is zone A's, its dark bank zone B's, and the reverse for B.
// The effort limit, the projection, K3, the attributes and the states read the chosen filters.
static int back_validation_span(apv_handle* h, hipStream_t st, void* const* wz, const BackSchedule& sch) {
    const apv_handle::ValSpan& vs = h->valspan;
    if (!vs.on) return APV_OK;
    const apv_stream* s = h->st;
    const size_t K = s->K, nV = s->nV;
    ValSpanArgs a;
    const LiveZones lz(s);
    a.zones = lz.nz;
    for (int i = 0; i < lz.nz; ++i) {
        const size_t z = lz.z[i];
        a.w[i] = wz[z];
        a.g_bright[i] = vs.d_G[z];
        a.g_dark[i] = vs.d_G[z ^ 1];
        a.phi[i] = vs.d_phi + z * K;
        a.bright[i] = vs.d_bright + z * K * nV;
        a.dark[i] = vs.d_dark + z * K * nV;
        a.src[i] = vs.d_src + z * K * nV;
    }
    a.emit = sch.span_quiet ? 0 : 1;
    std::string why;
    hipError_t e = apv_launch_validation_span(h->cfg.out_c128, s->K, s->nV, s->L, vs.Mv, a, st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    return APV_OK;
}

// FIR synthesis in place of K3 and K4: the hop's taps and the taps of the hop before it applied to the input signals in
// one launch, the target paths (pure delays) included, written where K4 writes; a second, small launch then makes this
// hop's taps and the newest J - 1 samples the next hop's.  Only the per-hop path reaches here (the chunked whole-signal
// path launches the synthesis of a whole chunk itself), after enqueue_front: the hop's samples lie behind `keep` older ones
// in the current input history, and the synthesis' own history alternates between two buffers with it.  Evaluation, the event
// and the copy back follow on the same stream.
static int back_fir_synthesis(apv_handle* h, hipStream_t st, void* pin_dst, const BackSchedule& sch) {
    apv_stream* s = h->st;
    char* const obuf = sch.result;
    const int J = s->taps, c = s->cur, f64 = s->f64;
    FirSynthArgs a = fir_synth_args(s, s->fs_taps, s->wtaps);
    FirSynthAdvance adv{};
    for (int i = 0; i < a.nz; ++i) { adv.cur[i] = a.cur[i]; adv.prev[i] = s->fs_taps[a.sig[i]]; }
    for (int g = 0; g < 2; ++g) {
        a.xhist[g] = s->fs_hist[c ^ 1][g];
        a.xhop[g] = static_cast<const char*>(s->xhist[c][g]) + (size_t)s->keep * s->esz;
        adv.old_hist[g] = a.xhist[g]; adv.xhop[g] = a.xhop[g]; adv.new_hist[g] = s->fs_hist[c][g];
    }
    a.out = obuf;
    adv.n_taps = (size_t)s->nV * J * s->L; adv.nz = a.nz; adv.J = J; adv.H = s->H;
    std::string why;
    if (s->fs_tm.ev[0]) SCHK(h, hipEventRecord(s->fs_tm.ev[0], st));
    hipError_t e = apv_launch_fir_synthesis(h->cfg.out_c128, f64, a, st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    if (s->fs_tm.ev[1]) SCHK(h, hipEventRecord(s->fs_tm.ev[1], st));
    SCHK(h, apv_launch_fir_synth_advance(h->cfg.out_c128, f64, adv, st));
    if (s->ev_on)
        if (int rc = enqueue_eval(h, st, obuf)) return rc;
    if (sch.spectra_free) SCHK(h, hipEventRecord(sch.spectra_free, st));
    if (!pin_dst) return APV_OK;
    SCHK(h, hipMemcpyAsync(pin_dst, obuf, hop_result_bytes(s), hipMemcpyDeviceToHost, st));     // samples + status: one copy
    return APV_OK;
}

// K3: output spectra in one launch: each live zone's nV*L filtered channels, then the target paths A_t, B_t
static int back_output_spectra(apv_handle* h, hipStream_t st, const HopSpectra& q, void* const* wz, const BackSchedule& sch) {
    const apv_stream* s = h->st;
    char* const ospec = sch.ospec;
    const int K = s->K, L = s->L;
    const size_t e2 = 2 * s->esz;
    const void* jin[4];
    const void* jw[4];
    const void* jt[4];
    void* jout[4];
    int jf[4], jtg[4], nj = 0;
    int oc = 0;     // output channel cursor
    const LiveZones lz(s);
    for (int i = 0; i < lz.nz; ++i) {
        const int z = lz.z[i];
        jin[nj] = (const char*)q.inspec + (size_t)z * K * e2; jw[nj] = wz[z]; jt[nj] = nullptr;
        jout[nj] = ospec + (size_t)oc * K * e2;
        jf[nj] = s->nV * L; jtg[nj] = 0; ++nj;
        oc += s->nV * L;
    }
    for (int z = 0; z < 2; ++z) {
        jin[nj] = (const char*)q.inspec + (size_t)z * K * e2; jw[nj] = nullptr; jt[nj] = s->tgt;
        jout[nj] = ospec + (size_t)oc * K * e2;
        jf[nj] = 0; jtg[nj] = L; ++nj;
        oc += L;
    }
    SCHK(h, apv_launch_apply_jobs(K, nj, jin, jw, jt, jout, jf, jtg, h->cfg.out_c128, s->f64, st));
    return APV_OK;
}

// Behind K3 on `st`: the event that says the spectra set has been read for the last time; then, on the tail stream where the
// schedule names one (it starts at that event), K4 (synthesis + overlap-add + emit), the evaluation and the copy back.
static int back_synthesis(apv_handle* h, hipStream_t st, void* pin_dst, const BackSchedule& sch) {
    apv_stream* s = h->st;
    char* const obuf = sch.result;
    if (sch.spectra_free) SCHK(h, hipEventRecord(sch.spectra_free, st));
    hipStream_t ts = st;
    if (sch.tail_stream) {
        ts = sch.tail_stream;
        SCHK(h, hipStreamWaitEvent(ts, sch.spectra_free, 0));
    }
    std::string why;
    hipError_t e = apv_launch_synthesis(s->f64, s->N, s->H, s->n_out, sch.ospec, s->K, 1, s->outov, obuf, ts, &why, s->out_group);
    if (e != hipSuccess) return launch_fail(h, e, why);
    if (s->ev_on)
        if (int rc = enqueue_eval(h, ts, obuf)) return rc;
    if (!pin_dst) return APV_OK;
    SCHK(h, hipMemcpyAsync(pin_dst, obuf, hop_result_bytes(s), hipMemcpyDeviceToHost, ts));         // samples + status: one copy
    if (sch.tail_stream) SCHK(h, hipEventRecord(sch.copied, ts));
    return APV_OK;
}

// Back half of a hop on stream `st`: spectra `q` -> per-bin filters (K5'-K10), the choice by validation contrast and the effort
// limit where the handle has them, their projection in a constrained stream, then
// output spectra (K3), synthesis and overlap-add (K4), or the FIR synthesis in their place; the emitted samples [n_out][H] and,
// behind them, the status words [2][K] land in pinned `pin_dst`.
static int enqueue_back(apv_handle* h, hipStream_t st, const HopSpectra& q, void* const* wz, void* const* lamz, void* pin_dst,
                        const BackSchedule& sch) {
    int rc = back_solve(h, st, q, wz, lamz, sch);
    if (rc == APV_OK) rc = back_validation_span(h, st, wz, sch);
    if (rc == APV_OK) rc = back_limit_effort(h, st, wz, sch);
    if (rc == APV_OK) rc = back_constrain(h, st, wz);
    if (rc != APV_OK) return rc;
    if (h->st->fir_synth) return back_fir_synthesis(h, st, pin_dst, sch);
    rc = back_output_spectra(h, st, q, wz, sch);
    if (rc == APV_OK) rc = back_synthesis(h, st, pin_dst, sch);
    return rc;
}

// everything one hop puts on the handle's stream, from the pinned input staging to the pinned output staging
static int enqueue_hop(apv_handle* h) {
    apv_stream* s = h->st;
    int rc = enqueue_front(h, h->stream, 0, s->pin_in);
    if (rc != APV_OK) return rc;
    return enqueue_back(h, h->stream, hop_spectra(s, 0), s->w, s->lam, s->pin_out, BackSchedule(s->out, s->outspec));
}

// run one hop whose input is already in the pinned staging; the output is left in the pinned staging
static int run_hop(apv_handle* h) {
    apv_stream* s = h->st;
    hipStream_t st = h->stream;
    const int H = s->H;
    if (s->period > 0 && s->live.hops_left == 0 && !win_low_rank(h)) {
        // replay the captured launch sequence of this phase; capture it the first time the phase comes up (a hop that adds a
        // correction tail runs the launches eagerly: the graphs stay those of a stream that was never updated)
        const int phase = (int)(s->hop % s->period);
        const int ring_before = s->ring_off, cur_before = s->cur;
        if (!s->execs[phase]) {
            hipGraph_t graph = nullptr;
            SCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            int rc = enqueue_hop(h);
            hipError_t ce = hipStreamEndCapture(st, &graph);
            if (rc != APV_OK || ce != hipSuccess) {
                if (graph) (void)hipGraphDestroy(graph);
                s->ring_off = ring_before;
                s->cur = cur_before;
                s->period = 0;                       // launch eagerly from now on
                rc = enqueue_hop(h);
                if (rc != APV_OK) return rc;
            } else {
                SCHK(h, hipGraphInstantiate(&s->execs[phase], graph, nullptr, nullptr, 0));
                (void)hipGraphDestroy(graph);
                SCHK(h, hipGraphLaunch(s->execs[phase], st));
            }
        } else {
            SCHK(h, hipGraphLaunch(s->execs[phase], st));
            // the host-side cursor moves exactly as enqueue_hop moves it
            s->cur ^= 1;
            s->ring_off = (s->ring_off + H) % s->N;
        }
    } else {
        int rc = enqueue_hop(h);
        if (rc != APV_OK) return rc;
    }
    s->hop++;
    if (s->win_fill_host < s->win_T) s->win_fill_host++;
    SCHK(h, hipStreamSynchronize(st));
    for (StageTimer* t : {&s->win_tm, &s->cf_tm, &s->fs_tm}) SCHK(h, t->read());
    return APV_OK;
}

// scan the per-bin status words of the hop: 1 = not positive definite (error, apvast.py:21-24), 2 = sweep cap reached
static int scan_hop_status(apv_handle* h, const int32_t* stat, long hop) {
    apv_stream* s = h->st;
    const int K = s->K;
    const bool runA = s->zones & 1, runB = s->zones & 2;
    int slow_zone = -1, slow_bin = -1;
    for (int z = 0; z < 2; ++z) {
        if (!(z ? runB : runA)) continue;
        for (int k = 0; k < K; ++k) {
            const int v = stat[(size_t)z * K + k];
            if (v == 1) {
                char buf[112];
                std::snprintf(buf, sizeof(buf), "Matrix is not positive definite (zone %c, bin %d, hop %ld)", z ? 'B' : 'A', k, hop);
                return apv_fail(h, APV_ERR_NOT_PD, buf);
            }
            if (v == 2 && slow_zone < 0) { slow_zone = z; slow_bin = k; }
        }
    }
    if (slow_zone >= 0) {
        s->not_converged++;
        char buf[128];
        std::snprintf(buf, sizeof(buf), "eigen-iteration did not converge (zone %c, bin %d, hop %ld); the outputs of this hop were written",
                      slow_zone ? 'B' : 'A', slow_bin, hop);
        return apv_fail(h, APV_ERR_NO_CONVERGE, buf);
    }
    return APV_OK;
}

// hops [first, first + n) of the caller's signals into pinned staging `pin` [n][2][H], [A | B] per hop, in the front-end precision
template <typename TI>
static void stage_hops(const apv_stream* s, const TI* h_in_A, const TI* h_in_B, int first, int n, void* pin) {
    const int H = s->H;
    for (int i = 0; i < n; ++i) {
        const TI* a = h_in_A + (size_t)(first + i) * H;
        const TI* b = h_in_B + (size_t)(first + i) * H;
        if (s->f64) {
            double* pi = (double*)pin + (size_t)i * 2 * H;
            for (int t = 0; t < H; ++t) { pi[t] = (double)a[t]; pi[H + t] = (double)b[t]; }
        } else {
            float* pi = (float*)pin + (size_t)i * 2 * H;
            for (int t = 0; t < H; ++t) { pi[t] = (float)a[t]; pi[H + t] = (float)b[t]; }
        }
    }
}

// the samples of hop i of n_hops from its result `res` into h_out.  Channel-major: h_out [n_hops][n_out][H].  Sample-major:
// h_out [n_out / L][n_hops * H][L], i.e. the hop's group g, a contiguous [H][L] block of the result, lands behind the same group of
// the hop before it (one straight copy per group)
template <typename TI>
static void copy_hop_out(const apv_stream* s, const void* res, int n_hops, int i, TI* h_out) {
    const size_t nout = (size_t)s->n_out * s->H;
    const size_t ngrp = s->out_group > 0 ? (size_t)s->n_out / s->out_group : 1, gsz = nout / ngrp;
    for (size_t g = 0; g < ngrp; ++g) {
        TI* dst = s->out_group > 0 ? h_out + (g * (size_t)n_hops + (size_t)i) * gsz : h_out + (size_t)i * nout;
        if (s->f64) {
            const double* po = (const double*)res + g * gsz;
            if (sizeof(TI) == sizeof(double)) std::memcpy(dst, po, gsz * sizeof(double));
            else for (size_t j = 0; j < gsz; ++j) dst[j] = (TI)po[j];
        } else {
            const float* po = (const float*)res + g * gsz;
            if (sizeof(TI) == sizeof(float)) std::memcpy(dst, po, gsz * sizeof(float));
            else for (size_t j = 0; j < gsz; ++j) dst[j] = (TI)po[j];
        }
    }
}

template <typename TI>
static int process_block_t(apv_handle* h, const TI* h_in_A, const TI* h_in_B, TI* h_out) {
    if (!h || !h_in_A || !h_in_B || !h_out) return apv_fail(h, APV_ERR_ARG, "null argument");
    apv_stream* s = h->st;
    if (!s) return apv_fail(h, APV_ERR_ARG, "apv_stream_init has not been called");
    SCHK(h, hipSetDevice(h->device));
    stage_hops(s, h_in_A, h_in_B, 0, 1, s->pin_in);
    if (s->ev_on)
        if (int rc = eval_begin_call(h, 1)) return rc;
    int rc = run_hop(h);
    if (rc != APV_OK) return rc;
    if (s->ev_on) s->ev_nrec = 1;
    copy_hop_out(s, s->pin_out, 1, 0, h_out);
    return scan_hop_status(h, hop_status_of(s, s->pin_out), s->hop - 1);
}

// ---- whole-signal path (apv_process_signal) ----

// the worst status of the hops of a call: the first APV_ERR_NO_CONVERGE, overridden by APV_ERR_NOT_PD, and its message
struct WorstStatus {
    int code = APV_OK;
    std::string msg;
    void note(const apv_handle* h, int r) {
        if (r == APV_ERR_NOT_PD && code != APV_ERR_NOT_PD) { code = r; msg = h->err; }
        if (r == APV_ERR_NO_CONVERGE && code == APV_OK) { code = r; msg = h->err; }
    }
};

// Every failure after the first enqueue leaves through here: the front stream, the `n_back` back streams and the tail stream are
// drained (kernels may still be reading the pinned staging and writing the result buffers), and the message says how far the call
// got -- the rings, histories and the hop counter have advanced by the hops ENQUEUED, of which only the hops DELIVERED reached h_out.
static int signal_bail(apv_handle* h, const hipStream_t* back, int n_back, int n_hops, long hop_first, long delivered, int code,
                       const std::string& msg) {
    apv_stream* s = h->st;
    (void)hipStreamSynchronize(s->front);
    for (int b = 0; b < n_back; ++b) (void)hipStreamSynchronize(back[b]);
    (void)hipStreamSynchronize(s->tail);
    char buf[192];
    const long enq = s->hop - hop_first;
    const long deliv = std::min<long>(delivered, enq);
    std::snprintf(buf, sizeof(buf), " [apv_process_signal: %ld of %d hops delivered, stream state advanced by %ld hops: restore it "
                  "with apv_set_state or re-initialise before continuing]", deliv, n_hops, enq);
    return apv_fail(h, code, msg + buf);
}

// The bookkeeping of one call of the pipeline or of the chunked driver: which chunks of the signal have been collected from the
// pinned staging, the worst status among their hops, and the two ways out of the call.  Chunk c lives in slot c mod n_slots of the
// staging `pin_out`, and `done[c mod n_slots]` says that it has been copied back.
template <typename TI>
struct SignalCall {
    apv_handle* h;
    int n_hops;
    TI* h_out;
    const hipStream_t* back;      // the back streams signal_bail drains
    int n_back;
    const hipEvent_t* done;
    const char* pin_out;
    int n_slots;
    int chunk, n_chunks;
    long hop_first;
    WorstStatus worst;
    int c_done = 0;               // chunks collected

    SignalCall(apv_handle* h_, int n_hops_, TI* h_out_, const hipStream_t* back_, int n_back_, const hipEvent_t* done_,
               const void* pin_out_, int n_slots_)
        : h(h_), n_hops(n_hops_), h_out(h_out_), back(back_), n_back(n_back_), done(done_), pin_out((const char*)pin_out_),
          n_slots(n_slots_), chunk(h_->st->sig_chunk), n_chunks((n_hops_ + chunk - 1) / chunk), hop_first(h_->st->hop) {}

    // hops of chunk c: results (one every hop_result_bytes) into h_out, and their status words scanned
    int collect(int c) {
        const apv_stream* s = h->st;
        const int base = c * chunk, nc = std::min(chunk, n_hops - base);
        hipError_t e = hipEventSynchronize(done[c % n_slots]);
        if (e != hipSuccess) return apv_fail(h, APV_ERR_HIP, std::string("apv_process_signal: ") + hipGetErrorString(e));
        const char* res = pin_out + (size_t)(c % n_slots) * chunk * hop_result_bytes(s);
        for (int i = 0; i < nc; ++i, res += hop_result_bytes(s)) {
            copy_hop_out(s, res, n_hops, base + i, h_out);
            worst.note(h, scan_hop_status(h, hop_status_of(s, res), hop_first + base + i));
        }
        return APV_OK;
    }
    int bail(int code, const std::string& msg) { return signal_bail(h, back, n_back, n_hops, hop_first, (long)c_done * chunk, code, msg); }
    int hipbail(hipError_t e) { return bail(APV_ERR_HIP, std::string("apv_process_signal: ") + hipGetErrorString(e)); }
    // Behind the driver's loop: the chunks still in flight (none of those behind a hop that was not positive definite), then
    // `leave_state` (the driver's: every stream drained, the stream state where the per-hop path expects it), then the call's status.
    template <typename F>
    int finish(F leave_state) {
        for (int c = c_done; c < n_chunks && (size_t)c * chunk < (size_t)(h->st->hop - hop_first); ++c) {
            if (int rc = collect(c)) return bail(rc, h->err);
            c_done = c + 1;
        }
        if (int rc = leave_state()) return bail(rc, h->err);
        if (worst.code == APV_ERR_NOT_PD) return bail(worst.code, worst.msg);     // the hops behind the failing one were not run
        if (worst.code != APV_OK) return apv_fail(h, worst.code, worst.msg);      // APV_ERR_NO_CONVERGE: every hop ran, every output is written
        return APV_OK;
    }
};

// what the whole-signal path needs beyond the per-hop path; allocated at its first call
static int signal_prepare(apv_handle* h) {
    apv_stream* s = h->st;
    if (s->sig_chunk > 0) return APV_OK;
    const size_t K = s->K, C = s->C, M = s->M, H = s->H, e1 = s->esz, e2 = 2 * s->esz;
    // hops per chunk of the whole-signal path (APV_SIGNAL_CHUNK: tuning aid, 4..64)
    static const int chunk_env = getenv("APV_SIGNAL_CHUNK") ? atoi(getenv("APV_SIGNAL_CHUNK")) : 0;
    const int chunk = (chunk_env >= 4 && chunk_env <= 64) ? chunk_env : 16;
    int rc;
    for (int p = 0; p < 4; ++p)
        if (!s->X1[p] && (rc = dalloc(h, &s->X1[p], (size_t)s->Kp * C, e2))) return rc;
    for (int z = 0; z < 2; ++z)
        if (!s->tspec1[z] && (rc = dalloc(h, &s->tspec1[z], K * M, e2))) return rc;
    if (!s->inspec1 && (rc = dalloc(h, &s->inspec1, 2 * K, e2))) return rc;
    if (!s->out1 && (rc = dalloc(h, &s->out1, hop_result_bytes(s), 1))) return rc;
    if (!s->outspec1 && (rc = dalloc(h, &s->outspec1, (size_t)s->n_out * K, e2))) return rc;
    if (s->fir_F > 0 && !s->xspec_chunk && (rc = dalloc(h, &s->xspec_chunk, (size_t)chunk * 2 * (s->fir_F / 2 + 1), e2))) return rc;
    // Front and tail at the DEFAULT stream priority.  (Rounds 2-4 ran them at the highest: their kernels are short or bandwidth-shaped
    // and everything downstream waits for them, and beside per-hop joint diagonalisations that is worth 3-6 % in a fresh process
    // -- but with priority streams the rate of the hop-by-hop schedule depends on how many streams the process created before:
    // 0.069 / 0.102 / 0.092 ms per hop at cfg3 after 0 / 3 / 5 earlier streams, against 0.074 / 0.071 / 0.074 at the default
    // priority (profiles/r04/cfg3_front_prio.txt).  The schedule with one joint-diagonalisation launch per chunk measures the same
    // either way.)
    if (!s->front) SCHK(h, s->own.stream(&s->front, hipStreamNonBlocking, 0));
    if (!s->tail) SCHK(h, s->own.stream(&s->tail, hipStreamNonBlocking, 0));
    for (int p = 0; p < 2; ++p) {
        if (!s->ev_copied[p]) SCHK(h, s->own.event(&s->ev_copied[p], hipEventDisableTiming));
        if (!s->ev_front[p]) SCHK(h, s->own.event(&s->ev_front[p], hipEventDisableTiming));
        if (!s->ev_back[p]) SCHK(h, s->own.event(&s->ev_back[p], hipEventDisableTiming));
        if (!s->ev_chunk[p]) SCHK(h, s->own.event(&s->ev_chunk[p], hipEventDisableTiming));
    }
    // two chunks of pinned staging: the host converts chunk c-1 while the device runs chunk c
    if (!s->sig_in) SCHK(h, s->own.pinned(&s->sig_in, e1 * 2 * chunk * 2 * H));
    if (!s->sig_out) {
        SCHK(h, s->own.pinned(&s->sig_out, 2 * chunk * hop_result_bytes(s)));
        std::memset(s->sig_out, 0, 2 * chunk * hop_result_bytes(s));
    }
    SCHK(h, hipStreamSynchronize(h->stream));               // the zero-fills above
    s->sig_chunk = chunk;
    return APV_OK;
}

// n_hops consecutive hops in one call.  Per hop the kernels, their order and their operands are those of
// apv_process_block, so the samples returned are the same bit for bit; what changes is the schedule: the front half of
// hop h+1 (nothing in it depends on hop h's filters) runs on a second stream beside the back half of hop h, the spectra
// alternating between two sets, and the host never waits for a hop: it stages and converts one chunk of hops while the
// device works on the next.
template <typename TI>
static int process_signal_chunked_t(apv_handle* h, int n_hops, const TI* h_in_A, const TI* h_in_B, TI* h_out);
template <typename TI>
static int process_signal_pipelined_t(apv_handle* h, int n_hops, const TI* h_in_A, const TI* h_in_B, TI* h_out);

// The whole-signal call of a stream with a statistics window: the hops one after the other through the per-hop path (its graphs
// included), so the samples are those of n_hops per-hop calls by construction.  (One statistics launch per chunk of hops is the
// follow-up named in DESIGN.md section 4.13.)  A constrained stream takes it where the chunked schedule does not apply (see
// process_signal_t) and where the projection or the FIR synthesis is being timed launch by launch.
template <typename TI>
static int process_signal_hops_t(apv_handle* h, int n_hops, const TI* h_in_A, const TI* h_in_B, TI* h_out) {
    apv_stream* s = h->st;
    SCHK(h, hipSetDevice(h->device));
    WorstStatus worst;                                       // first APV_ERR_NO_CONVERGE: every hop still runs
    if (s->ev_on)
        if (int rc = eval_begin_call(h, n_hops)) return rc;
    for (int i = 0; i < n_hops; ++i) {
        stage_hops(s, h_in_A, h_in_B, i, 1, s->pin_in);
        int rc = run_hop(h);
        if (rc != APV_OK) return rc;
        if (s->ev_on) s->ev_nrec = i + 1;
        copy_hop_out(s, s->pin_out, n_hops, i, h_out);
        rc = scan_hop_status(h, hop_status_of(s, s->pin_out), s->hop - 1);
        if (rc != APV_OK && rc != APV_ERR_NO_CONVERGE) return rc;
        worst.note(h, rc);
    }
    if (worst.code != APV_OK) return apv_fail(h, worst.code, worst.msg);
    return APV_OK;
}

template <typename TI>
static int process_signal_t(apv_handle* h, int n_hops, const TI* h_in_A, const TI* h_in_B, TI* h_out) {
    if (!h || !h_in_A || !h_in_B || !h_out) return apv_fail(h, APV_ERR_ARG, "null argument");
    apv_stream* s = h->st;
    if (!s) return apv_fail(h, APV_ERR_ARG, "apv_stream_init has not been called");
    if (n_hops < 0) return apv_fail(h, APV_ERR_ARG, "n_hops must be >= 0");
    if (n_hops == 0) return APV_OK;
    // K1 as one fast-convolution segment (responses of 64 taps or more): a chunk of hops per launch (process_signal_chunked_t);
    // direct-form K1 (shorter responses, APV_FIR_DIRECT) and partitioned K1 keep the hop-by-hop pipeline (process_signal_pipelined_t).  A
    // constrained stream takes the chunked schedule or the plain hop loop: never the pipeline, which does not order the projections
    // of consecutive hops; and the hop loop when its projection or synthesis is timed (the switches promise un-captured per-hop
    // launches, tools/bench_filter_constraint.py and tools/bench_fir_synthesis.py read one time per hop).
    // An evaluated stream takes the hop loop too: its output histories and totals make consecutive hops sequential.
    const bool chunked = !explicit_stats(s) && !s->ev_on && s->fir_F > 0 && s->fir_np == 1 && !(s->taps > 0 && (s->cf_tm.ev[0] || s->fs_tm.ev[0]));
    const long hop_before = s->hop;
    int rc;
    if (chunked) rc = process_signal_chunked_t<TI>(h, n_hops, h_in_A, h_in_B, h_out);
    else if (explicit_stats(s) || s->taps > 0 || s->ev_on) rc = process_signal_hops_t<TI>(h, n_hops, h_in_A, h_in_B, h_out);
    else rc = process_signal_pipelined_t<TI>(h, n_hops, h_in_A, h_in_B, h_out);
    s->sched[0] = chunked ? (int32_t)(s->hop - hop_before) : 0;
    s->sched[1] = chunked ? 0 : (int32_t)(s->hop - hop_before);
    return rc;
}

// the two spectra sets (and the result buffers that follow them) of the hop-by-hop pipeline
struct PipelineSets {
    int set = 0, last_set = 0;
    bool released[2] = {true, true};                         // nothing reads either set yet
    bool out_idle[2] = {true, true};                         // no copy of either result buffer pending
};

// one hop of the pipeline: front half on the front stream into the next set, back half on the handle's stream, synthesis and copy
// back (to pinned `pin_dst`) on the tail stream
static int pipeline_hop(apv_handle* h, PipelineSets& ps, const void* pin_src, void* pin_dst) {
    apv_stream* s = h->st;
    const int set = ps.set;
    hipStream_t back = h->stream;
    // hop h-2 has to be done with this set before the analysis transforms write it
    int rc = enqueue_front(h, s->front, set, pin_src, ps.released[set] ? nullptr : s->ev_back[set]);
    if (rc != APV_OK) return rc;
    SIGCHK(h, hipEventRecord(s->ev_front[set], s->front));
    SIGCHK(h, hipStreamWaitEvent(back, s->ev_front[set], 0));
    // the output buffers follow the set; hop h-2's synthesis and copy have to be through before this hop writes them
    if (!ps.out_idle[set]) SIGCHK(h, hipStreamWaitEvent(back, s->ev_copied[set], 0));
    BackSchedule sch(set ? s->out1 : s->out, set ? s->outspec1 : s->outspec);    // the output buffers follow the set
    sch.spectra_free = s->ev_back[set];          // recorded after K3, the set's last reader
    sch.tail_stream = s->tail;
    sch.copied = s->ev_copied[set];
    rc = enqueue_back(h, back, hop_spectra(s, set), s->w, s->lam, pin_dst, sch);
    if (rc != APV_OK) return rc;
    ps.out_idle[set] = false;
    ps.released[set] = false;
    ps.last_set = set;
    ps.set ^= 1;
    s->hop++;
    return APV_OK;
}

// behind the last hop: the state arrays and apv_process_block live in set 0, so the last hop's spectra are brought there; then
// every stream of the pipeline is drained
static int pipeline_leave_state(apv_handle* h, const PipelineSets& ps) {
    apv_stream* s = h->st;
    hipStream_t back = h->stream;
    if (ps.last_set == 1) {
        const size_t K = s->K, C = s->C, M = s->M, e2 = 2 * s->esz;
        for (int p = 0; p < 4; ++p) SIGCHK(h, hipMemcpyAsync(s->X[p], s->X1[p], (size_t)s->Kp * C * e2, hipMemcpyDeviceToDevice, back));
        for (int z = 0; z < 2; ++z) SIGCHK(h, hipMemcpyAsync(s->tspec[z], s->tspec1[z], K * M * e2, hipMemcpyDeviceToDevice, back));
        SIGCHK(h, hipMemcpyAsync(s->inspec, s->inspec1, 2 * K * e2, hipMemcpyDeviceToDevice, back));
    }
    SIGCHK(h, hipStreamSynchronize(s->front));
    SIGCHK(h, hipStreamSynchronize(back));
    SIGCHK(h, hipStreamSynchronize(s->tail));
    return APV_OK;
}

// the hop-by-hop pipeline of the whole-signal call (direct-form or partitioned K1, no statistics window, no constraint)
template <typename TI>
static int process_signal_pipelined_t(apv_handle* h, int n_hops, const TI* h_in_A, const TI* h_in_B, TI* h_out) {
    apv_stream* s = h->st;
    SCHK(h, hipSetDevice(h->device));
    int rc = signal_prepare(h);
    if (rc != APV_OK) return rc;
    const int H = s->H, chunk = s->sig_chunk;
    const size_t e1 = s->esz;
    hipStream_t back = h->stream;
    PipelineSets ps;
    // chunk c of the signal lives in half c & 1 of the pinned staging
    SignalCall<TI> call(h, n_hops, h_out, &back, 1, s->ev_chunk, s->sig_out, 2);
    for (int c = 0; c < call.n_chunks && call.worst.code != APV_ERR_NOT_PD; ++c) {
        const int base = c * chunk, nc = std::min(chunk, n_hops - base);
        // this half was collected when chunk c-2's event came in
        stage_hops(s, h_in_A, h_in_B, base, nc, (char*)s->sig_in + (size_t)(c & 1) * chunk * 2 * H * e1);
        for (int i = 0; i < nc; ++i) {
            const size_t slot = (size_t)(c & 1) * chunk + i;
            rc = pipeline_hop(h, ps, (const char*)s->sig_in + slot * 2 * H * e1, (char*)s->sig_out + slot * hop_result_bytes(s));
            if (rc != APV_OK) return call.bail(rc, h->err);
        }
        {
            const hipError_t e = hipEventRecord(s->ev_chunk[c & 1], s->tail);   // every front and back half is upstream of some copy
            if (e != hipSuccess) return call.hipbail(e);
        }
        if (c > 0) {
            if ((rc = call.collect(c - 1)) != APV_OK) return call.bail(rc, h->err);
            call.c_done = c;
        }
    }
    return call.finish([&] { return pipeline_leave_state(h, ps); });
}

// what the chunked whole-signal path needs beyond signal_prepare(); allocated at its first call
static int chunk_prepare(apv_handle* h) {
    apv_stream* s = h->st;
    if (s->ck_RL > 0) return APV_OK;
    int rc = signal_prepare(h);
    if (rc != APV_OK) return rc;
    const size_t K = s->K, C = s->C, M = s->M, L = s->L, e1 = s->esz, e2 = 2 * s->esz;
    const int chunk = s->sig_chunk;
    const size_t RL = (size_t)s->N - s->H + (size_t)chunk * s->H;
    for (int q = 0; q < 2; ++q) {
        for (int p = 0; p < 4; ++p)
            if ((rc = dalloc(h, &s->ck_resp[q][p], C * RL, e1))) return rc;
        for (int z = 0; z < 2; ++z)
            if ((rc = dalloc(h, &s->ck_tresp[q][z], M * RL, e1))) return rc;
        if ((rc = dalloc(h, &s->ck_in[q], 2 * RL, e1))) return rc;
        if ((rc = dalloc(h, &s->ck_tspec[q], (size_t)2 * chunk * K * M, e2))) return rc;
        for (int b = 0; b < CK_NB; ++b) SCHK(h, s->own.event(&s->ck_backdone[q][b], hipEventDisableTiming));
    }
    for (int b = 0; b < CK_NB; ++b) SCHK(h, s->own.event(&s->ck_k3[b], hipEventDisableTiming));
    for (int z = 0; z < 2; ++z) {
        if ((rc = dalloc(h, &s->ck_wall[z], (size_t)chunk * K * s->nV * L, wsz(h)))) return rc;
        if ((rc = dalloc(h, &s->ck_lamall[z], (size_t)chunk * K * L, lsz(h)))) return rc;
    }
    for (int b = 0; b + 1 < CK_NB; ++b) {
        for (int z = 0; z < 2; ++z) {
            if ((rc = dalloc(h, &s->ck_w[b][z], K * s->nV * L, wsz(h)))) return rc;
            if ((rc = dalloc(h, &s->ck_lam[b][z], K * L, lsz(h)))) return rc;
        }
        {
            const apv_config& c = h->cfg;
            const size_t spill = apv_gevd_spill_bytes((int)L, (int)K, c.compute_dtype, c.reg_mode, c.reg_bright, c.sweep_tol2, c.n_zones == 3 ? 2 : 1);
            if (spill > 0 && (rc = dalloc(h, &s->ck_spill[b], spill, 1))) return rc;
        }
        // (the back streams themselves are made by chunk_begin, and only where the hop-by-hop schedule runs: the
        // runtime deals a process's streams over four hardware queues, and a stream that exists takes part whether it is used or not)
    }
    for (int q = 0; q < CK_NS; ++q) SCHK(h, s->own.event(&s->ck_done[q], hipEventDisableTiming));
    SCHK(h, s->own.pinned(&s->ck_pin_in, e1 * CK_NS * chunk * 2 * s->H));
    SCHK(h, s->own.pinned(&s->ck_pin_out, (size_t)CK_NS * chunk * hop_result_bytes(s)));
    std::memset(s->ck_pin_out, 0, (size_t)CK_NS * chunk * hop_result_bytes(s));
    for (int p = 0; p < 4; ++p)
        if ((rc = dalloc(h, &s->ck_X[p], (size_t)2 * chunk * s->Kp * C, e2))) return rc;
    if ((rc = dalloc(h, &s->ck_inspec, (size_t)2 * chunk * 2 * K, e2))) return rc;
    if ((rc = dalloc(h, &s->ck_out, (size_t)2 * chunk * hop_result_bytes(s), 1))) return rc;
    if ((rc = dalloc(h, &s->ck_ospec, (size_t)2 * chunk * s->n_out * K, e2))) return rc;
    if (s->taps > 0) {
        for (int z = 0; z < 2; ++z)
            if ((s->zones & (1 << z)) && (rc = dalloc(h, &s->ck_taps[z], (size_t)chunk * s->nV * s->taps * L, lsz(h)))) return rc;
        SCHK(h, s->own.event(&s->ck_wallfree, hipEventDisableTiming));
    }
    if (s->fir_synth)
        for (int q = 0; q < 2; ++q)
            for (int g = 0; g < 2; ++g)
                if ((rc = dalloc(h, &s->ck_xrow[q][g], (size_t)s->taps - 1 + (size_t)chunk * s->H, e1))) return rc;
    SCHK(h, hipStreamSynchronize(h->stream));               // the zero-fills above
    s->ck_RL = (int)RL;
    return APV_OK;
}

// One call of the chunked whole-signal path (process_signal_chunked_t): its constants, the back streams with their filter sets,
// where the stream stood when the call began and where the call's last hop ran.
struct ChunkCall {
    apv_handle* h;
    apv_stream* s;
    // a constrained stream: ONE projection launch per chunk behind the chunk's joint diagonalisations, whose filters all go to
    // ck_wall; with FIR synthesis ONE synthesis launch per chunk in place of K3 and K4 (chunk_back_batched, chunk_constrained_tail)
    bool cons, fir;
    // the chunk's joint diagonalisations as one launch where the kernel that will run takes several hops (order 16, absolute loading,
    // no diagnostics); elsewhere hop by hop on the back streams
    bool batched;
    size_t hop_w, hop_lam, hop_taps;             // bytes of one hop's filters, eigenvalues and taps of one zone program
    hipStream_t bs[CK_NB];                       // back streams, with the filters and eigenvalues each writes
    void* wset[CK_NB][2];
    void* lset[CK_NB][2];
    long hop_first;
    int n_hops = 0;                              // hops of the call
    int ring_first, cur_first;
    int last_par = 0, last_nc = 0, last_b = 0;   // chunk parity, hops and back stream of the last hop enqueued
};

static int chunk_begin(apv_handle* h, ChunkCall& k) {
    apv_stream* s = h->st;
    k.h = h;
    k.s = s;
    k.cons = s->taps > 0;
    k.fir = s->fir_synth != 0;
    k.hop_w = (size_t)s->K * s->nV * s->L * wsz(h);
    k.hop_lam = (size_t)s->K * s->L * lsz(h);
    k.hop_taps = (size_t)s->nV * s->taps * s->L * lsz(h);
    {
        GevdParams probe = apv_base_params(h);
        probe.x_c128 = s->f64;
        probe.x_group = s->xg;
        probe.n_hops = 2;
        static const bool force_generic = getenv("APV_FORCE_GENERIC") != nullptr;
        k.batched = !force_generic && apv_gevd16m_takes_hops(probe, h->cfg.compute_dtype, true);
    }
    if (!k.batched)
        for (int b = 0; b + 1 < CK_NB; ++b)
            if (!s->ck_back[b]) SCHK(h, s->own.stream(&s->ck_back[b], hipStreamNonBlocking));
    for (int b = 0; b < CK_NB; ++b) {
        k.bs[b] = (b && s->ck_back[b - 1]) ? s->ck_back[b - 1] : h->stream;
        for (int z = 0; z < 2; ++z) {
            k.wset[b][z] = b ? s->ck_w[b - 1][z] : s->w[z];
            k.lset[b][z] = b ? s->ck_lam[b - 1][z] : s->lam[z];
        }
    }
    k.hop_first = s->hop;
    k.ring_first = s->ring_off;
    k.cur_first = s->cur;
    return APV_OK;
}

// the spectra set of hop i of a chunk of parity par
static HopSpectra chunk_set(const apv_stream* s, int par, int i) {
    HopSpectra q;
    const size_t idx = (size_t)par * s->sig_chunk + i, K = s->K, e2 = 2 * s->esz;
    for (int p = 0; p < 4; ++p) q.X[p] = (char*)s->ck_X[p] + idx * (size_t)s->Kp * s->C * e2;
    for (int z = 0; z < 2; ++z) q.tspec[z] = (char*)s->ck_tspec[z] + idx * K * s->M * e2;
    q.inspec = (char*)s->ck_inspec + idx * 2 * K * e2;
    return q;
}

// ... and its result and output-spectra slots: every hop of the two chunks in flight has its own, and the chunk's results go back
// in one copy (chunk_copy_back)
static BackSchedule chunk_slots(const apv_stream* s, int par, int i) {
    const size_t slot = (size_t)par * s->sig_chunk + i;
    return BackSchedule((char*)s->ck_out + slot * hop_result_bytes(s), (char*)s->ck_ospec + slot * (size_t)s->n_out * s->K * 2 * s->esz);
}

// ... and its slots of ck_wall / ck_lamall
static void chunk_filters(const ChunkCall& k, int i, void** wz, void** lz) {
    for (int z = 0; z < 2; ++z) {
        wz[z] = (char*)k.s->ck_wall[z] + i * k.hop_w;
        lz[z] = (char*)k.s->ck_lamall[z] + i * k.hop_lam;
    }
}

// the filters of the chunk's nc hops (ck_wall) projected in place, their taps to ck_taps: one launch on `st`
static int chunk_project(const ChunkCall& k, hipStream_t st, int nc) {
    apv_handle* h = k.h;
    const apv_stream* s = k.s;
    void *cw[2], *ct[2];
    const LiveZones lz(s);
    for (int i = 0; i < lz.nz; ++i) { cw[i] = s->ck_wall[lz.z[i]]; ct[i] = s->ck_taps[lz.z[i]]; }
    std::string why;
    hipError_t e = apv_launch_constrain_filters_hops(h->cfg.out_c128, s->N, s->taps, s->nV, s->L, lz.nz, cw, ct, nc, k.hop_w / wsz(h),
                                                     k.hop_taps / lsz(h), st, &why);
    if (e != hipSuccess) return launch_fail(h, e, why);
    return APV_OK;
}

// the FIR synthesis of the chunk's nc hops into their result slots: one launch on `st`, hop i fading from the taps of hop i - 1
// (hop 0 from fs_taps), and behind it the last hop's taps to fs_taps for the next chunk or call
static int chunk_synthesis(const ChunkCall& k, hipStream_t st, int par, int nc) {
    apv_handle* h = k.h;
    const apv_stream* s = k.s;
    FirSynthArgs a = fir_synth_args(s, s->fs_taps, s->ck_taps);
    for (int g = 0; g < 2; ++g) {
        a.xhist[g] = s->ck_xrow[par][g];
        a.xhop[g] = (const char*)s->ck_xrow[par][g] + (size_t)(s->taps - 1) * s->esz;
    }
    a.out = (char*)s->ck_out + (size_t)par * s->sig_chunk * hop_result_bytes(s);
    a.n_hops = nc; a.hop_taps = k.hop_taps / lsz(h); a.hop_x = s->H; a.hop_out = hop_result_bytes(s);
    std::string why;
    hipError_t e = apv_launch_fir_synthesis(h->cfg.out_c128, s->f64, a, st, &why);
    const LiveZones lz(s);
    for (int i = 0; i < lz.nz && e == hipSuccess; ++i)
        e = hipMemcpyAsync(s->fs_taps[lz.z[i]], (char*)s->ck_taps[lz.z[i]] + (size_t)(nc - 1) * k.hop_taps, k.hop_taps,
                           hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return launch_fail(h, e, why);
    return APV_OK;
}

// Front half of the whole chunk c (nc hops, staged in pinned `pin`) on the front stream: input side, K1, analysis, weighting.
static int chunk_front(ChunkCall& k, int c, int nc, const char* pin) {
    apv_handle* h = k.h;
    apv_stream* s = k.s;
    const int N = s->N, H = s->H, M = s->M, C = s->C, P = s->P, f64 = s->f64, chunk = s->sig_chunk, RL = s->ck_RL, par = c & 1;
    // the spectra sets and linear buffers of this parity were last read by the back halves of chunk c - 2
    if (c >= 2)
        for (int b = 0; b < CK_NB; ++b) SIGCHK(h, hipStreamWaitEvent(s->front, s->ck_backdone[par][b], 0));
    // ... and, in a constrained stream, by what follows the chunk's projection: K3, or the synthesis reading the input rows
    if (k.cons && c >= 2) SIGCHK(h, hipStreamWaitEvent(s->front, s->ck_done[(c - 2) % CK_NS], 0));
    SIGCHK(h, apv_launch_fir_chunk_spectra(f64, s->fir_F, P, H, nc, s->xhist[s->cur][0], s->xhist[s->cur][1], pin, s->xspec_chunk, s->front));
    // heads of the linear buffers: the newest N - H samples before the chunk, from the rings (first chunk) or from the tail
    // of the previous chunk's buffers
    {
        const int prev = par ^ 1, prev_nc = chunk;               // every chunk but the last is full
        auto head = [&](void* dst, const void* ring, const void* lin_prev, int rows) -> hipError_t {
            if (c == 0) return apv_launch_rows_copy(f64, rows, N - H, dst, RL, 0, RL, ring, N, (H + k.ring_first) % N, N, s->front);
            return apv_launch_rows_copy(f64, rows, N - H, dst, RL, 0, RL, lin_prev, RL, prev_nc * H, RL, s->front);
        };
        for (int p = 0; p < 4; ++p) SIGCHK(h, head(s->ck_resp[par][p], s->resp[p], s->ck_resp[prev][p], C));
        for (int z = 0; z < 2; ++z) SIGCHK(h, head(s->ck_tresp[par][z], s->tresp[z], s->ck_tresp[prev][z], M));
        SIGCHK(h, head(s->ck_in[par], s->inblk, s->ck_in[prev], 2));
    }
    {
        const void* oh[2] = {s->xhist[s->cur][0], s->xhist[s->cur][1]};
        void* nh[2] = {s->xhist[s->cur ^ 1][0], s->xhist[s->cur ^ 1][1]};
        SIGCHK(h, apv_launch_chunk_inputs(f64, P, H, N, nc, s->pad, RL, oh, nh, pin, s->ck_in[par], s->front));
        s->cur ^= 1;
    }
    if (k.fir) {
        // the synthesis' linear input rows [J - 1 samples before the chunk | the chunk]: the head from the synthesis' history
        // (first chunk) or from the tail of the other parity's rows (the chunk before: always full)
        const void* head[2] = {c == 0 ? s->fs_hist[k.cur_first][0] : s->ck_xrow[par ^ 1][0],
                               c == 0 ? s->fs_hist[k.cur_first][1] : s->ck_xrow[par ^ 1][1]};
        void* rows[2] = {s->ck_xrow[par][0], s->ck_xrow[par][1]};
        SIGCHK(h, apv_launch_fir_synth_rows(f64, s->taps, H, nc, head, c == 0 ? 0 : (size_t)chunk * H, pin, rows, s->front));
    }
    {
        // K1: every (hop, channel) of the chunk in one launch
        const K1Jobs j = k1_jobs(s, s->ck_resp[par], s->ck_tresp[par], s->xspec_chunk);
        SIGCHK(h, apv_launch_fir_fft_chunk(f64, s->fir_F, 6, j.jh, j.jx, (long)(2 * (s->fir_F / 2 + 1)), j.jr, j.jc, P, H, RL, N - H, nc, s->front));
    }
    if (s->live.hops_left > 0) {
        // the chunk's share of the pending correction tails, on the samples the per-hop path would add them to
        void* dst[6] = {s->ck_resp[par][0], s->ck_resp[par][1], s->ck_resp[par][2], s->ck_resp[par][3], s->ck_tresp[par][0],
                        s->ck_tresp[par][1]};
        if (int rc = apv_live_apply(h, s->live, P, C, M, f64, dst, nc * H, nc * H, RL, N - H, RL, s->front)) return rc;
        apv_live_advance(s->live, nc);
    }
    {
        // K2: every analysis transform of the chunk in one launch; hop i's block starts i H samples into the rows
        const AnalysisJobs j = analysis_jobs(s, s->ck_resp[par], s->ck_tresp[par], s->ck_in[par], chunk_set(s, par, 0));
        std::string why;
        hipError_t e = apv_launch_stft_analysis_chunk(f64, N, j.nj, j.jx, j.jch, j.jspec, j.jsc, j.jsk, RL, H, j.jhop, nc, s->front, &why);
        if (e != hipSuccess) return launch_fail(h, e, why);
    }
    for (int i = 0; i < nc; ++i)
        if (int rc = enqueue_weighting(h, chunk_set(s, par, i), s->front)) return rc;
    SIGCHK(h, hipEventRecord(s->ev_front[par], s->front));
    return APV_OK;
}

// hop i of the chunk behind its filters (and their projection): K3 on `st`, K4 where `sch` says
static int chunk_hop_outputs(const ChunkCall& k, hipStream_t st, int par, int i, const BackSchedule& sch) {
    void *wz[2], *lz[2];
    chunk_filters(k, i, wz, lz);
    int rc = back_output_spectra(k.h, st, chunk_set(k.s, par, i), wz, sch);
    if (rc == APV_OK) rc = back_synthesis(k.h, st, nullptr, sch);
    return rc;
}

// Back halves of chunk c, regime (a): the joint diagonalisations of the whole chunk as ONE launch (blockIdx.z = hop), then output
// spectra and synthesis hop by hop.  A hop's 2050 waves are two per SIMD, all head and tail; every input of the
// sixteen exists once the chunk's transforms have ended, and sixteen hops are a launch of the headline's size.  Same values per bin.
// A constrained stream projects the chunk's filters behind the launch, on the same stream.
static int chunk_back_batched(ChunkCall& k, int c, int nc) {
    apv_handle* h = k.h;
    apv_stream* s = k.s;
    const int par = c & 1;
    const size_t e2 = 2 * s->esz;
    hipStream_t b0 = k.bs[0];
    SIGCHK(h, hipStreamWaitEvent(b0, s->ev_front[par], 0));
    if (c >= 2) SIGCHK(h, hipStreamWaitEvent(b0, s->ck_done[(c - 2) % CK_NS], 0));        // the result slots of this parity are free
    {
        char* const obuf0 = (char*)s->ck_out + (size_t)par * s->sig_chunk * hop_result_bytes(s);
        GevdParams p = fused_gevd_params(h, chunk_set(s, par, 0), s->ck_wall, s->ck_lamall, reinterpret_cast<int32_t*>(obuf0 + hop_out_bytes(s)));
        p.yield_issue = 1;
        p.n_hops = nc;
        p.hop_X = (size_t)s->Kp * s->C * e2;
        p.hop_d = (size_t)s->K * s->M * e2;
        p.hop_w = k.hop_w;
        p.hop_lam = k.hop_lam;
        p.hop_status = hop_result_bytes(s);
        p.span.last_hop = nc - 1;        // the span's outputs are those of the chunk's last hop
        std::string why;
        hipError_t e = apv_launch_gevd(p, h->cfg.compute_dtype, true, b0, &why);
        if (e != hipSuccess) return launch_fail(h, e, why);
    }
    // the effort limit of the whole chunk in one launch; the outputs are those of the chunk's last hop (the chunks follow one
    // another on this stream, so the call's last hop writes last)
    if (h->effort.on)
        if (int rc = effort_launch(h, b0, s->ck_wall, nc, k.hop_w / wsz(h), nc - 1)) return rc;
    if (k.cons)
        if (int rc = chunk_project(k, b0, nc)) return rc;
    if (k.fir) {
        // K3 and K4 are not launched: the chunk's synthesis writes the result slots, and the tail stream only copies them back
        if (int rc = chunk_synthesis(k, b0, par, nc)) return rc;
        SIGCHK(h, hipEventRecord(s->ck_k3[0], b0));
        SIGCHK(h, hipStreamWaitEvent(s->tail, s->ck_k3[0], 0));
        SIGCHK(h, hipEventRecord(s->ck_backdone[par][0], b0));
        k.last_par = par; k.last_nc = nc; k.last_b = 0;
        s->hop += nc;
        return APV_OK;
    }
    for (int i = 0; i < nc; ++i) {
        BackSchedule sch = chunk_slots(s, par, i);
        sch.spectra_free = s->ck_k3[0];
        sch.tail_stream = s->tail;
        if (int rc = chunk_hop_outputs(k, b0, par, i, sch)) return rc;
        if (i + 1 == nc) SIGCHK(h, hipEventRecord(s->ck_backdone[par][0], b0));
        k.last_par = par; k.last_nc = nc; k.last_b = 0;
        s->hop++;
    }
    return APV_OK;
}

// Back halves of chunk c, regime (b): hop by hop, alternating between the back streams (configurations the batched launch does
// not take).
static int chunk_back_hops(ChunkCall& k, int c, int nc) {
    apv_handle* h = k.h;
    apv_stream* s = k.s;
    const int par = c & 1;
    for (int i = 0; i < nc; ++i) {
        const int b = (int)((s->hop - k.hop_first) % CK_NB);
        if (i < CK_NB) {
            SIGCHK(h, hipStreamWaitEvent(k.bs[b], s->ev_front[par], 0));
            // the result slots of this parity are being copied back for chunk c - 2 (still in flight: the host collects two
            // chunks behind)
            if (c >= 2) SIGCHK(h, hipStreamWaitEvent(k.bs[b], s->ck_done[(c - 2) % CK_NS], 0));
            // a constrained stream: the tail stream is done with the filters and taps of chunk c - 1 (one set of each)
            if (k.cons && c >= 1) SIGCHK(h, hipStreamWaitEvent(k.bs[b], s->ck_wallfree, 0));
        }
        // Every hop of the two chunks in flight has result and output-spectra slots of its own, so a back stream never waits
        // for the tail stream inside a chunk: its next diagonalisation follows the previous one directly.
        BackSchedule sch = chunk_slots(s, par, i);
        sch.yield_issue = 1;
        sch.lspill = b > 0 ? s->ck_spill[b - 1] : nullptr;
        // the hops of the back streams run side by side: the span's outputs are written by the call's last hop alone
        sch.span_quiet = s->hop - k.hop_first != k.n_hops - 1;
        int rc;
        if (k.cons) {
            // the back stream runs the joint diagonalisation alone, into the hop's own slots of ck_wall / ck_lamall: the
            // projections share one taps buffer and the cross-fade needs hop order, both of which the tail stream keeps
            // (chunk_constrained_tail)
            void *wz[2], *lz[2];
            chunk_filters(k, i, wz, lz);
            rc = back_solve(h, k.bs[b], chunk_set(s, par, i), wz, lz, sch);
        } else {
            sch.spectra_free = s->ck_k3[b];                  // recorded after K3: the tail stream starts the synthesis there
            sch.tail_stream = s->tail;
            rc = enqueue_back(h, k.bs[b], chunk_set(s, par, i), k.wset[b], k.lset[b], nullptr, sch);
        }
        if (rc != APV_OK) return rc;
        if (i + CK_NB >= nc) SIGCHK(h, hipEventRecord(s->ck_backdone[par][b], k.bs[b]));   // this stream's last hop of the chunk
        k.last_par = par; k.last_nc = nc; k.last_b = b;
        s->hop++;
    }
    return APV_OK;
}

// A constrained stream in regime (b): the tail stream, behind the chunk's last diagonalisation on every back stream, runs the
// chunk's projection, then K3 + K4 hop by hop, or the chunk's FIR synthesis.
static int chunk_constrained_tail(const ChunkCall& k, int par, int nc) {
    apv_handle* h = k.h;
    const apv_stream* s = k.s;
    for (int b = 0; b < CK_NB; ++b) SIGCHK(h, hipStreamWaitEvent(s->tail, s->ck_backdone[par][b], 0));
    // the effort limit of the chunk's hops in one launch ahead of the projection (the back streams ran the diagonalisations alone)
    int rc = h->effort.on ? effort_launch(h, s->tail, s->ck_wall, nc, k.hop_w / wsz(h), nc - 1) : APV_OK;
    if (rc == APV_OK) rc = chunk_project(k, s->tail, nc);
    if (rc == APV_OK && k.fir) rc = chunk_synthesis(k, s->tail, par, nc);
    for (int i = 0; i < nc && !k.fir && rc == APV_OK; ++i) rc = chunk_hop_outputs(k, s->tail, par, i, chunk_slots(s, par, i));
    if (rc != APV_OK) return rc;
    SIGCHK(h, hipEventRecord(s->ck_wallfree, s->tail));
    return APV_OK;
}

// the chunk's results in ONE copy behind its last synthesis (16 hops: 6.4 MB at cfg3)
static int chunk_copy_back(const ChunkCall& k, int c, int nc) {
    apv_handle* h = k.h;
    const apv_stream* s = k.s;
    const size_t chunk_bytes = (size_t)s->sig_chunk * hop_result_bytes(s);
    SIGCHK(h, hipMemcpyAsync((char*)s->ck_pin_out + (size_t)(c % CK_NS) * chunk_bytes, (char*)s->ck_out + (size_t)(c & 1) * chunk_bytes,
                             (size_t)nc * hop_result_bytes(s), hipMemcpyDeviceToHost, s->tail));
    SIGCHK(h, hipEventRecord(s->ck_done[c % CK_NS], s->tail)); // every front and back half of the chunk is upstream of this copy
    return APV_OK;
}

// Behind the last chunk, every stream drained: the state n_hops per-hop calls would have left.
static int chunk_leave_state(ChunkCall& k) {
    apv_handle* h = k.h;
    apv_stream* s = k.s;
    const int N = s->N, H = s->H, K = s->K, M = s->M, C = s->C, f64 = s->f64, RL = s->ck_RL, J = s->taps;
    const size_t e1 = s->esz, e2 = 2 * s->esz;
    SIGCHK(h, hipStreamSynchronize(s->front));
    for (int b = 1; b < CK_NB; ++b) SIGCHK(h, hipStreamSynchronize(k.bs[b]));
    SIGCHK(h, hipStreamSynchronize(s->tail));
    SIGCHK(h, hipStreamSynchronize(k.bs[0]));
    const long done = s->hop - k.hop_first;
    if (done <= 0) return APV_OK;
    hipStream_t st = k.bs[0];
    const int last_par = k.last_par, last_nc = k.last_nc;
    // rings: the last hop's block, written at the ring offset the per-hop path (and its captured graphs) expects after
    // `done` more hops
    s->ring_off = (int)((k.ring_first + done * H) % N);
    const int src0 = (last_nc - 1) * H;
    for (int p = 0; p < 4; ++p) SIGCHK(h, apv_launch_rows_copy(f64, C, N, s->resp[p], N, s->ring_off, N, s->ck_resp[last_par][p], RL, src0, RL, st));
    for (int z = 0; z < 2; ++z) SIGCHK(h, apv_launch_rows_copy(f64, M, N, s->tresp[z], N, s->ring_off, N, s->ck_tresp[last_par][z], RL, src0, RL, st));
    SIGCHK(h, apv_launch_rows_copy(f64, 2, N, s->inblk, N, s->ring_off, N, s->ck_in[last_par], RL, src0, RL, st));
    // histories: the per-hop path alternates the two buffers every hop
    const int cur_expected = k.cur_first ^ (int)(done & 1);
    if (s->cur != cur_expected) {
        const size_t hb = ((size_t)s->P - 1 + H + s->pad) * e1;
        for (int g = 0; g < 2; ++g) SIGCHK(h, hipMemcpyAsync(s->xhist[cur_expected][g], s->xhist[s->cur][g], hb, hipMemcpyDeviceToDevice, st));
        s->cur = cur_expected;
    }
    // the last hop's spectra, filters and eigenvalues where the state arrays and the per-hop path keep them
    const HopSpectra q = chunk_set(s, last_par, last_nc - 1);
    for (int p = 0; p < 4; ++p) SIGCHK(h, hipMemcpyAsync(s->X[p], q.X[p], (size_t)s->Kp * C * e2, hipMemcpyDeviceToDevice, st));
    for (int z = 0; z < 2; ++z) SIGCHK(h, hipMemcpyAsync(s->tspec[z], q.tspec[z], (size_t)K * M * e2, hipMemcpyDeviceToDevice, st));
    SIGCHK(h, hipMemcpyAsync(s->inspec, q.inspec, (size_t)2 * K * e2, hipMemcpyDeviceToDevice, st));
    if (k.batched || k.cons) {
        void *wz[2], *lz[2];
        chunk_filters(k, last_nc - 1, wz, lz);
        for (int z = 0; z < 2; ++z) {
            SIGCHK(h, hipMemcpyAsync(s->w[z], wz[z], k.hop_w, hipMemcpyDeviceToDevice, st));
            SIGCHK(h, hipMemcpyAsync(s->lam[z], lz[z], k.hop_lam, hipMemcpyDeviceToDevice, st));
        }
        // a constrained stream: the last hop's taps, and the newest J - 1 input samples in the history buffer the next per-hop
        // call reads (fs_taps took the last hop's taps behind the chunk's synthesis)
        for (int z = 0; z < 2 && k.cons; ++z)
            if (s->zones & (1 << z))
                SIGCHK(h, hipMemcpyAsync(s->wtaps[z], (char*)s->ck_taps[z] + (size_t)(last_nc - 1) * k.hop_taps, k.hop_taps, hipMemcpyDeviceToDevice, st));
        for (int g = 0; g < 2 && k.fir && J > 1; ++g)
            SIGCHK(h, hipMemcpyAsync(s->fs_hist[s->cur][g], (char*)s->ck_xrow[last_par][g] + (size_t)last_nc * H * e1, (size_t)(J - 1) * e1,
                                     hipMemcpyDeviceToDevice, st));
    } else if (k.last_b != 0) {
        for (int z = 0; z < 2; ++z) {
            SIGCHK(h, hipMemcpyAsync(s->w[z], k.wset[k.last_b][z], k.hop_w, hipMemcpyDeviceToDevice, st));
            SIGCHK(h, hipMemcpyAsync(s->lam[z], k.lset[k.last_b][z], k.hop_lam, hipMemcpyDeviceToDevice, st));
        }
    }
    SIGCHK(h, hipStreamSynchronize(st));
    return APV_OK;
}

// n_hops consecutive hops in one call, a CHUNK of hops at a time (responses of >= 64 taps, i.e. K1 by fast convolution).
//
// Nothing in the front half of a hop (input histories, K1, analysis transforms, perceptual weighting) depends on any hop's
// filters, and the whole signal is in hand: the front halves of the 16 hops of a chunk are therefore THREE launches -- the input
// side (hops into the input-block buffers, histories as after the chunk), K1 for every (hop, channel), the analysis transform
// of every (hop, channel) -- into linear buffers [channel][N - H + 16 H] whose head is the tail of the previous chunk's, and
// into one spectra set per hop.  Each (hop, channel) is the workgroup the per-hop launch would have run, on the same operands in
// the same order: the samples returned are those of apv_process_block bit for bit.  The back halves (joint diagonalisation,
// output spectra) of consecutive hops are independent of each other and alternate between two streams with their own filters,
// output spectra and result buffers, so two hops' diagonalisations share the chip (four waves per SIMD instead of two);
// synthesis, overlap-add and the copy back stay in hop order on the tail stream.  The host stages chunk c + 1 and collects
// chunk c - 1 while the device runs chunk c.  On return the rings, histories, spectra, filters and counters are what n_hops
// calls of apv_process_block would have left (apv_get_state, the per-hop entry points and their captured graphs carry on).
template <typename TI>
static int process_signal_chunked_t(apv_handle* h, int n_hops, const TI* h_in_A, const TI* h_in_B, TI* h_out) {
    apv_stream* s = h->st;
    SCHK(h, hipSetDevice(h->device));
    int rc = chunk_prepare(h);
    if (rc != APV_OK) return rc;
    ChunkCall k;
    if ((rc = chunk_begin(h, k)) != APV_OK) return rc;
    k.n_hops = n_hops;
    const int H = s->H, chunk = s->sig_chunk;
    // staging slot c mod 3 holds chunk c
    SignalCall<TI> call(h, n_hops, h_out, k.bs, CK_NB, s->ck_done, s->ck_pin_out, CK_NS);
    for (int c = 0; c < call.n_chunks && call.worst.code != APV_ERR_NOT_PD; ++c) {
        const int base = c * chunk, nc = std::min(chunk, n_hops - base);
        char* const pin = (char*)s->ck_pin_in + (size_t)(c % CK_NS) * chunk * 2 * H * s->esz;
        stage_hops(s, h_in_A, h_in_B, base, nc, pin);        // staging slot c mod 3: chunk c - 3 was collected an iteration ago
        rc = chunk_front(k, c, nc, pin);
        if (rc == APV_OK) rc = k.batched ? chunk_back_batched(k, c, nc) : chunk_back_hops(k, c, nc);
        if (rc == APV_OK && k.cons && !k.batched) rc = chunk_constrained_tail(k, c & 1, nc);
        if (rc == APV_OK) rc = chunk_copy_back(k, c, nc);
        if (rc != APV_OK) return call.bail(rc, h->err);
        // the host collects TWO chunks behind: while it waits for chunk c - 2 and copies it out, chunks c - 1 and c are queued on
        // the device, so the front half of chunk c runs beside the back halves of chunk c - 1 whatever the host is doing
        if (c > 1) {
            if ((rc = call.collect(c - 2)) != APV_OK) return call.bail(rc, h->err);
            call.c_done = c - 1;
        }
    }
    return call.finish([&] { return chunk_leave_state(k); });
}

// spectra of one bank for the fast-convolution K1: cm [n_ch][P] channel-major -> spec [fir_np][n_ch][fir_F/2 + 1] (one segment: the
// whole response; partitioned: taps [q H, (q + 1) H) of every channel, partition-major)
static int bank_spectra(apv_handle* h, const void* cm, int n_ch, void* spec) {
    const apv_stream* s = h->st;
    const int np = s->fir_np, P = s->P, H = s->H;
    const size_t Kf = (size_t)s->fir_F / 2 + 1;
    std::string why;
    hipError_t e = hipSuccess;
    for (int q = 0; q < np && e == hipSuccess; ++q) {
        const int taps = np == 1 ? P : std::min(H, P - q * H);
        e = apv_launch_fir_spectra_part(s->f64, s->fir_F, n_ch, (const char*)cm + (size_t)q * (np == 1 ? 0 : H) * s->esz, P, taps,
                                        (char*)spec + (size_t)q * Kf * n_ch * 2 * s->esz, h->stream, &why);
    }
    if (e != hipSuccess) return launch_fail(h, e, why);
    return APV_OK;
}

extern "C" {

int apv_stream_init(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B,
                    int32_t reference_index_A, int32_t reference_index_B, int32_t modeling_delay) {
    if (!h || !h_rir_A || !h_rir_B) return apv_fail(h, APV_ERR_ARG, "null argument");
    const apv_config& c = h->cfg;
    const int N = c.block_size, H = c.hop_size;
    {
        std::string why;
        if (!apv_stft_size_ok(N, &why)) return apv_fail(h, APV_ERR_ARG, why);
    }
    if (c.frontend < 0 || c.frontend > 2) return apv_fail(h, APV_ERR_ARG, "cfg.frontend must be 0 (follow compute_dtype), 1 (float32) or 2 (float64)");
    if (c.out_layout != 0 && c.out_layout != 1) return apv_fail(h, APV_ERR_ARG, "cfg.out_layout must be 0 (channel-major) or 1 (sample-major groups)");
    const int f64 = frontend_f64(c);
    if (f64 && N > 4096) return apv_fail(h, APV_ERR_ARG, "float64 front-end: block_size <= 4096 (double-precision FFT in LDS)");
    if (H < 1 || H > N) return apv_fail(h, APV_ERR_ARG, "hop_size must be in 1..block_size");
    if (c.n_bins != N / 2 + 1) return apv_fail(h, APV_ERR_ARG, "streaming handle needs n_bins == block_size/2 + 1");
    if (rir_len < 1 || modeling_delay < 0 || modeling_delay >= rir_len) return apv_fail(h, APV_ERR_ARG, "rir_len / modeling_delay out of range");
    if (reference_index_A < 0 || reference_index_A >= c.n_srcs || reference_index_B < 0 || reference_index_B >= c.n_srcs)
        return apv_fail(h, APV_ERR_ARG, "reference index out of range");
    if (c.n_zones < 1 || c.n_zones > 3) return apv_fail(h, APV_ERR_ARG, "n_zones is a bit mask: 1 = A, 2 = B, 3 = both");
    if (h->filter_taps > 0) {
        std::string why;
        if (h->filter_taps > N) return apv_fail(h, APV_ERR_ARG, "filter taps (apv_stream_set_filter_taps) must not exceed block_size");
        if (modeling_delay >= h->filter_taps) return apv_fail(h, APV_ERR_ARG, "modeling_delay must be below the filter taps (apv_stream_set_filter_taps)");
        if (!apv_constrain_size_ok(c.out_c128, N, &why)) return apv_fail(h, APV_ERR_ARG, why);
    }
    if (h->synthesis == APV_SYNTH_FIR && h->filter_taps < 1)
        return apv_fail(h, APV_ERR_ARG, "FIR synthesis (apv_stream_set_synthesis) needs the filter taps of apv_stream_set_filter_taps");
    if (h->eval_Pv > 0) {
        const int nzp = ((c.n_zones & 1) ? 1 : 0) + ((c.n_zones & 2) ? 1 : 0);
        if ((long)nzp * (2 * (long)h->eval_ranks.size() + 1) > 65535)
            return apv_fail(h, APV_ERR_ARG, "evaluation (apv_stream_set_evaluation): at most 65535 pressure sets");
        if (h->eval_rv[0].size() != (size_t)h->eval_Pv * c.n_srcs * h->eval_Mv)
            return apv_fail(h, APV_ERR_ARG, "evaluation (apv_stream_set_evaluation): the responses were sized for another n_srcs");
    }
    if (h->valspan.on && (h->eval_Pv <= 0 || h->eval_Mv != h->valspan.Mv))
        return apv_fail(h, APV_ERR_ARG, "validation span (apv_stream_set_validation_span): the transfer functions were sized for the "
                                        "validation microphones of another apv_stream_set_evaluation");
    if (h->eval_spectra) {
        if (h->eval_Pv <= 0)
            return apv_fail(h, APV_ERR_ARG, "evaluation spectra (apv_stream_set_evaluation_spectra) need the evaluation stage of apv_stream_set_evaluation");
        if (N > 4096)
            return apv_fail(h, APV_ERR_ARG, "evaluation spectra (apv_stream_set_evaluation_spectra): block_size <= 4096 (the spectra are float64 "
                                            "whatever the stream's precision, and the double-precision FFT in LDS stops there)");
        const int nzp = ((c.n_zones & 1) ? 1 : 0) + ((c.n_zones & 2) ? 1 : 0);
        std::string why;
        if (!apv_eval_spectra_size_ok(N, H, nzp, (int)h->eval_ranks.size(), h->eval_Mv, &why)) return apv_fail(h, APV_ERR_ARG, why);
    }
    if (h->eval_detect_C > 0) {
        if (!h->eval_spectra)
            return apv_fail(h, APV_ERR_ARG, "evaluation detectability (apv_stream_set_evaluation_detectability) needs the per-bin spectra of "
                                            "apv_stream_set_evaluation_spectra");
        if (h->eval_detect_G2.size() != (size_t)c.n_bins * h->eval_detect_C)
            return apv_fail(h, APV_ERR_ARG, "evaluation detectability (apv_stream_set_evaluation_detectability): the table was sized for another n_bins");
        const int nzp = ((c.n_zones & 1) ? 1 : 0) + ((c.n_zones & 2) ? 1 : 0);
        std::string why;
        if (!apv_eval_detect_size_ok(N, nzp, (int)h->eval_ranks.size(), h->eval_Mv, h->eval_detect_C, &why)) return apv_fail(h, APV_ERR_ARG, why);
    }
    SCHK(h, hipSetDevice(h->device));
    apv_stream_free(h);
    apv_stream* s = new apv_stream();                       // value-initialised: every scalar, pointer and array member starts at zero
    h->st = s;
    // an init that fails from here on leaves no half-built stream behind
    struct Guard { apv_handle* h; bool ok; ~Guard() { if (!ok) apv_stream_free(h); } } built{h, false};
    s->N = N; s->H = H; s->K = N / 2 + 1; s->L = c.n_srcs; s->M = c.n_mics; s->C = s->L * s->M;
    s->P = rir_len; s->nV = c.n_ranks; s->zones = c.n_zones; s->pad = apv_fir_pad();
    s->f64 = f64; s->esz = f64 ? 8 : 4;
    s->ring_off = 0; s->cur = 0;
    const int nz = ((s->zones & 1) ? 1 : 0) + ((s->zones & 2) ? 1 : 0);
    s->n_out = nz * s->nV * s->L + 2 * s->L;
    s->out_group = c.out_layout == 1 ? s->L : 0;
    s->Kp = (s->K + 7) / 8 * 8;
    s->win_T = h->stat_hops > 1 ? h->stat_hops : 1;
    s->fg_beta = h->stat_forgetting;
    s->taps = h->filter_taps;
    // (a windowed or forgetting stream does not launch the fused kernel that reads grouped spectra: its slabs stay bin-major)
    s->xg_default = explicit_stats(s) ? 1 : apv_gevd_reads_groups(apv_base_params(h), h->cfg.compute_dtype, f64 != 0);
    s->xg = s->xg_default;
    const int L = s->L, M = s->M, C = s->C, P = s->P, K = s->K;
    const size_t e1 = s->esz, e2 = 2 * s->esz;
    int rc;
    // RIRs: host (P, L, M) float64 C-order -> device [P][m*L + l] in the front-end precision
    std::vector<double> tmp((size_t)P * C), ttmp((size_t)P * M);
    for (int z = 0; z < 2; ++z) {
        const double* src = z ? h_rir_B : h_rir_A;
        const int ref = z ? reference_index_B : reference_index_A;
        for (int p = 0; p < P; ++p)
            for (int l = 0; l < L; ++l)
                for (int m = 0; m < M; ++m) tmp[(size_t)p * C + m * L + l] = src[((size_t)p * L + l) * M + m];
        // target RIR: reference loudspeaker delayed by modeling_delay (apvast.py:102-112)
        std::fill(ttmp.begin(), ttmp.end(), 0.0);
        for (int p = modeling_delay; p < P; ++p)
            for (int m = 0; m < M; ++m) ttmp[(size_t)p * M + m] = src[((size_t)(p - modeling_delay) * L + ref) * M + m];
        if ((rc = dalloc(h, &s->rir[z], (size_t)P * C, e1))) return rc;
        if ((rc = dalloc(h, &s->trir[z], (size_t)P * M, e1))) return rc;
        if ((rc = upload(h, f64, s->rir[z], tmp))) return rc;
        if ((rc = upload(h, f64, s->trir[z], ttmp))) return rc;
    }
    // long responses: the hop's convolution goes through the frequency domain (fir_fft_kernel); APV_FIR_DIRECT keeps the
    // direct form on the matrix cores (A/B switch)
    s->fir_F = getenv("APV_FIR_DIRECT") == nullptr ? apv_fir_fft_size(f64, P, H) : 0;
    s->fir_np = 1;
    s->keep = P - 1;
    if (s->fir_F == 0 && getenv("APV_FIR_DIRECT") == nullptr) {
        // too long for one segment in LDS: uniformly partitioned, partitions of H taps in segments of 2 H samples
        const int np = apv_fir_partitions(f64, P, H);
        if (np > 0) {
            s->fir_F = 2 * H;
            s->fir_np = np;
            s->keep = np * H;
        }
    }
    if (s->fir_F > 0) {
        const int F = s->fir_F, np = s->fir_np;
        const size_t Kf = (size_t)F / 2 + 1;
        ApvOwned scratch;
        void* cm = nullptr;                                  // [C][P] channel-major copy of one bank, set-up only
        SCHK(h, scratch.zeroed(&cm, (size_t)C * P, e1, h->stream));
        std::vector<double> tr((size_t)C * P);
        for (int z = 0; z < 2; ++z) {
            const double* src = z ? h_rir_B : h_rir_A;
            const int ref = z ? reference_index_B : reference_index_A;
            if ((rc = dalloc(h, &s->rirspec[z], (size_t)np * Kf * C, e2))) return rc;
            if ((rc = dalloc(h, &s->trirspec[z], (size_t)np * Kf * M, e2))) return rc;
            for (int p = 0; p < P; ++p)
                for (int l = 0; l < L; ++l)
                    for (int m = 0; m < M; ++m) tr[(size_t)(m * L + l) * P + p] = src[((size_t)p * L + l) * M + m];
            if ((rc = upload(h, f64, cm, tr))) return rc;
            if ((rc = bank_spectra(h, cm, C, s->rirspec[z]))) return rc;
            SCHK(h, hipStreamSynchronize(h->stream));
            std::fill(tr.begin(), tr.end(), 0.0);
            for (int p = modeling_delay; p < P; ++p)
                for (int m = 0; m < M; ++m) tr[(size_t)m * P + p] = src[((size_t)(p - modeling_delay) * L + ref) * M + m];
            if ((rc = upload(h, f64, cm, tr))) return rc;
            if ((rc = bank_spectra(h, cm, M, s->trirspec[z]))) return rc;
            SCHK(h, hipStreamSynchronize(h->stream));
        }
        if ((rc = dalloc(h, &s->xspec, (size_t)np * 2 * Kf, e2))) return rc;
    }
    const size_t hist = (size_t)s->keep + H + s->pad;
    for (int b = 0; b < 2; ++b)
        for (int g = 0; g < 2; ++g)
            if ((rc = dalloc(h, &s->xhist[b][g], hist, e1))) return rc;
    for (int p = 0; p < 4; ++p) {
        if ((rc = dalloc(h, &s->resp[p], (size_t)C * N, e1))) return rc;
        if ((rc = dalloc(h, &s->X[p], (size_t)s->Kp * C, e2))) return rc;
    }
    for (int z = 0; z < 2; ++z) {
        if ((rc = dalloc(h, &s->tresp[z], (size_t)M * N, e1))) return rc;
        if ((rc = dalloc(h, &s->tspec[z], (size_t)K * M, e2))) return rc;
        if ((rc = dalloc(h, &s->w[z], (size_t)K * s->nV * L, wsz(h)))) return rc;
        if ((rc = dalloc(h, &s->lam[z], (size_t)K * L, lsz(h)))) return rc;
    }
    if ((rc = dalloc(h, &s->inblk, (size_t)2 * N, e1))) return rc;
    if ((rc = dalloc(h, &s->inspec, (size_t)2 * K, e2))) return rc;
    if ((rc = dalloc(h, &s->tgt, (size_t)L * K, e2))) return rc;
    if ((rc = dalloc(h, &s->outspec, (size_t)s->n_out * K, e2))) return rc;
    if ((rc = dalloc(h, &s->outov, (size_t)s->n_out * N, e1))) return rc;
    {
        // samples, then the status words [zone A | zone B] of the hop: one copy back
        char* outbuf = nullptr;
        if ((rc = dalloc(h, &outbuf, hop_result_bytes(s), 1))) return rc;
        s->out = outbuf;
        s->status[0] = reinterpret_cast<int32_t*>(outbuf + hop_out_bytes(s));
        s->status[1] = s->status[0] + K;
    }
    if (explicit_stats(s)) {
        // the ring of per-hop Gram matrices (forgetting: the one accumulator slot) and the sums the joint diagonalisation reads,
        // in the precision it runs in (orders above 64: float64 whatever compute_dtype is)
        s->win_c128 = (c.compute_dtype == APV_F64 || L > APV_MAX_N) ? 1 : 0;
        const size_t ce = s->win_c128 ? 16 : 8, E = apv_statwin_slot_elems(L);
        const size_t ring_bytes = (size_t)s->win_T * K * E * ce;
        for (int z = 0; z < 2; ++z) {
            if (!(s->zones & (1 << z))) continue;
            hipError_t e = s->own.device(&s->win_ring[z], ring_bytes);
            if (e != hipSuccess) {
                char buf[192];
                std::snprintf(buf, sizeof(buf), "statistics %s: the ring of %d hop(s) needs %zu bytes per zone program (%d of them): %s",
                              s->fg_beta > 0.0 ? "accumulator" : "window", s->win_T, ring_bytes, nz, hipGetErrorString(e));
                return apv_fail(h, APV_ERR_HIP, buf);
            }
            SCHK(h, hipMemsetAsync(s->win_ring[z], 0, ring_bytes, h->stream));
            if ((rc = dalloc(h, &s->win_RB[z], (size_t)K * L * L, ce))) return rc;
            if ((rc = dalloc(h, &s->win_RD[z], (size_t)K * L * L, ce))) return rc;
            if ((rc = dalloc(h, &s->win_r[z], (size_t)K * L, ce))) return rc;
        }
        if (s->fg_beta == 0.0 && (rc = dalloc(h, &s->win_ctr, 2))) return rc;
        // Forgetting at order 64 with M < L: the first hops hold fewer than L rows and the later ones geometrically weighted rows,
        // neither of which the float32 sweeps of kernels_gevd64.hip resolve (see win_low_rank).  No threshold in beta or in the
        // hop count separates the two: such a stream keeps every solve off that kernel, so its launch sequence is one and captured.
        s->fg_no_gevd64 = s->fg_beta > 0.0 && s->win_c128 && M < L && apv_gevd64_eligible(L, c.reg_mode, c.reg_bright, c.sweep_tol2);
        if (getenv("APV_STAT_WINDOW_TIMING") != nullptr)
            for (int i = 0; i < 2; ++i) SCHK(h, s->own.event(&s->win_tm.ev[i], hipEventDefault));
    }
    if (s->taps > 0) {
        for (int z = 0; z < 2; ++z)
            if ((s->zones & (1 << z)) && (rc = dalloc(h, &s->wtaps[z], (size_t)s->nV * s->taps * L, lsz(h)))) return rc;
        SCHK(h, apv_stft_prepare(N, c.out_c128));           // the projection runs in the filters' precision
        if (getenv("APV_FILTER_CONSTRAINT_TIMING") != nullptr)
            for (int i = 0; i < 2; ++i) SCHK(h, s->own.event(&s->cf_tm.ev[i], hipEventDefault));
    }
    if (h->synthesis == APV_SYNTH_FIR) {
        s->fir_synth = 1;
        s->fs_ref = reference_index_A;
        s->fs_delay = modeling_delay;
        for (int z = 0; z < 2; ++z)
            if ((s->zones & (1 << z)) && (rc = dalloc(h, &s->fs_taps[z], (size_t)s->nV * s->taps * L, lsz(h)))) return rc;
        for (int b = 0; b < 2; ++b)
            for (int g = 0; g < 2; ++g)
                if ((rc = dalloc(h, &s->fs_hist[b][g], (size_t)s->taps - 1, e1))) return rc;
        if (getenv("APV_FIR_SYNTHESIS_TIMING") != nullptr)
            for (int i = 0; i < 2; ++i) SCHK(h, s->own.event(&s->fs_tm.ev[i], hipEventDefault));
    }
    if (h->eval_Pv > 0) {
        // evaluation stage: per zone program that runs, the pressure sets [bright of E ranks][dark of E ranks][target]; bright and
        // target through the responses of the program's own zone, dark through the other zone's
        const int Pv = h->eval_Pv, Mv = h->eval_Mv, E = (int)h->eval_ranks.size(), nfilt = nz * s->nV;
        s->ev_on = 1; s->ev_Pv = Pv; s->ev_Mv = Mv; s->ev_E = E; s->ev_Z = nz;
        s->ev_sets = nz * (2 * E + 1); s->ev_nhist = nz * (E + 1);
        std::vector<int32_t> map((size_t)4 * s->ev_sets, 0), hsrc(s->ev_nhist, 0);
        int zi = 0;
        for (int z = 0; z < 2; ++z) {
            if (!(s->zones & (1 << z))) continue;
            for (int e = 0; e <= E; ++e) {
                int grp = nfilt + z;                         // e = E: the program's target output A_t / B_t
                if (e < E) {
                    const auto it = std::find(h->rank_list.begin(), h->rank_list.end(), h->eval_ranks[e]);
                    if (it == h->rank_list.end()) return apv_fail(h, APV_ERR_ARG, "evaluation: a rank that is not in the handle's rank list");
                    grp = zi * s->nV + (int)(it - h->rank_list.begin());
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
        for (int z = 0; z < 2; ++z) {
            if ((rc = dalloc(h, &s->ev_rv[z], h->eval_rv[z].size()))) return rc;
            SCHK(h, hipMemcpyAsync(s->ev_rv[z], h->eval_rv[z].data(), sizeof(double) * h->eval_rv[z].size(), hipMemcpyHostToDevice, h->stream));
        }
        if ((rc = dalloc(h, &s->ev_map, map.size()))) return rc;
        if ((rc = dalloc(h, &s->ev_hsrc, hsrc.size()))) return rc;
        SCHK(h, hipMemcpyAsync(s->ev_map, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice, h->stream));
        SCHK(h, hipMemcpyAsync(s->ev_hsrc, hsrc.data(), sizeof(int32_t) * hsrc.size(), hipMemcpyHostToDevice, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));            // map, hsrc go out of scope
        for (int b = 0; b < 2; ++b)
            if ((rc = dalloc(h, &s->ev_hist[b], (size_t)s->ev_nhist * (Pv - 1) * L, e1))) return rc;
        if ((rc = dalloc(h, &s->ev_p, (size_t)s->ev_sets * H * Mv))) return rc;
        if ((rc = dalloc(h, &s->ev_tot, (size_t)nz * (3 * E + 1) * Mv))) return rc;
        if ((rc = dalloc(h, &s->ev_ctl, 4))) return rc;
        SCHK(h, apv_eval_pressure_prepare(f64, Pv, H, L));
        if (h->eval_spectra) {
            s->es_on = 1;
            if ((rc = dalloc(h, &s->es_ring, (size_t)s->ev_sets * Mv * N))) return rc;
            if ((rc = dalloc(h, &s->es_spec, (size_t)K * s->ev_sets * Mv, 2 * sizeof(double)))) return rc;
            if ((rc = dalloc(h, &s->es_tot, (size_t)nz * (3 * E + 1) * K * Mv))) return rc;
            SCHK(h, apv_stft_prepare(N, 1));                 // the float64 plan, beside the stream's own where that is float32
        }
        if (h->eval_detect_C > 0) {
            const int Cn = h->eval_detect_C;
            s->ed_on = 1; s->ed_C = Cn;
            s->ed_Cs = h->eval_detect_Cs; s->ed_Ca = h->eval_detect_Ca; s->ed_Leff = h->eval_detect_Leff;
            std::vector<double> gt((size_t)Cn * K);
            for (int k = 0; k < K; ++k)
                for (int i = 0; i < Cn; ++i) gt[(size_t)i * K + k] = h->eval_detect_G2[(size_t)k * Cn + i];
            if ((rc = dalloc(h, &s->ed_G2T, gt.size()))) return rc;
            SCHK(h, hipMemcpyAsync(s->ed_G2T, gt.data(), sizeof(double) * gt.size(), hipMemcpyHostToDevice, h->stream));
            SCHK(h, hipStreamSynchronize(h->stream));        // gt goes out of scope
            if ((rc = dalloc(h, &s->ed_quiet, (size_t)K))) return rc;
            if ((rc = dalloc(h, &s->ed_curves, (size_t)K * nz * Mv))) return rc;
            if ((rc = dalloc(h, &s->ed_part, (size_t)apv_eval_detect_chunks(N, nz, E, Mv) * nz * 2 * E * Mv))) return rc;
            if ((rc = dalloc(h, &s->ed_tot, (size_t)nz * 6 * E * Mv))) return rc;
            if ((rc = dalloc(h, &s->ed_ctl, 3))) return rc;
            SCHK(h, apv_launch_eval_detect_quiet(N, Cn, s->ed_G2T, s->ed_Cs, s->ed_Ca, s->ed_Leff, s->ed_quiet, h->stream));
        }
    }
    // target filter spectra: rfft of a unit impulse at tap modeling_delay of the A reference loudspeaker
    // (apvast.py:389-390, 418, 422: the same filter serves A_t and B_t)
    std::vector<double> tg((size_t)L * K * 2, 0.0);
    const double PI = 3.14159265358979323846;
    for (int k = 0; k < K; ++k) {
        // exact at the multiples of a quarter turn, like an FFT of the unit impulse
        const long q = ((long)k * modeling_delay) % N;
        double cr = std::cos(-2.0 * PI * (double)q / (double)N), ci = std::sin(-2.0 * PI * (double)q / (double)N);
        if ((4 * q) % N == 0) {
            const int quarter = (int)((4 * q) / N);
            cr = quarter == 0 ? 1.0 : quarter == 2 ? -1.0 : 0.0;
            ci = quarter == 1 ? -1.0 : quarter == 3 ? 1.0 : 0.0;
        }
        tg[((size_t)reference_index_A * K + k) * 2] = cr;
        tg[((size_t)reference_index_A * K + k) * 2 + 1] = ci;
    }
    if ((rc = upload(h, f64, s->tgt, tg))) return rc;
    s->h_status.assign((size_t)2 * K, 0);
    SCHK(h, s->own.pinned(&s->pin_in, e1 * 2 * H));
    SCHK(h, s->own.pinned(&s->pin_out, hop_result_bytes(s)));
    std::memset(s->pin_out, 0, hop_result_bytes(s));
    // the launch sequence of a hop depends on (ring_off, cur) only: ring_off has period N / gcd(N, H), cur period 2
    {
        int a = N, b = H;
        while (b) { const int t = a % b; a = b; b = t; }
        int per = N / a;
        if (per % 2) per *= 2;
        // (the statistics window adds no phase: its ring position is two device words that a kernel of the hop advances.  Timed
        // statistics launches -- a measuring aid -- run eagerly: their events are read after every hop)
        // (the FIR synthesis alternates its history buffers with cur, whose period of 2 is part of per already)
        s->period = (per <= 16 && getenv("APV_NO_GRAPH") == nullptr && !s->win_tm.ev[0] && !s->cf_tm.ev[0] && !s->fs_tm.ev[0]) ? per : 0;
        s->execs.assign(s->period > 0 ? s->period : 0, nullptr);
    }
    s->hop = 0;
    SCHK(h, apv_stft_prepare(N, f64));
    SCHK(h, hipStreamSynchronize(h->stream));
    built.ok = true;
    return APV_OK;
}

int apv_stream_set_stat_hops(apv_handle* h, int32_t n_hops) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_stat_hops: the stream is initialised (the ring of hops is sized there)");
    if (n_hops < 1 || n_hops > APV_MAX_STAT_HOPS) return apv_fail(h, APV_ERR_ARG, "statistics window: between 1 and 64 hops");
    if (n_hops > 1 && h->stat_forgetting > 0.0)
        return apv_fail(h, APV_ERR_ARG, "apv_stream_set_stat_hops: exponential forgetting is set (a window and forgetting exclude each other)");
    h->stat_hops = n_hops;
    return APV_OK;
}

int apv_stream_set_filter_taps(apv_handle* h, int32_t J) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_filter_taps: the stream is initialised (the taps buffer is allocated there)");
    if (J < 0 || (h->cfg.block_size > 0 && J > h->cfg.block_size))
        return apv_fail(h, APV_ERR_ARG, "filter taps: 0 (off) or between 1 and block_size");
    h->filter_taps = J;
    return APV_OK;
}

int apv_stream_set_synthesis(apv_handle* h, int32_t mode) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_synthesis: the stream is initialised (its buffers are allocated there)");
    if (mode != APV_SYNTH_WOLA && mode != APV_SYNTH_FIR)
        return apv_fail(h, APV_ERR_ARG, "synthesis: APV_SYNTH_WOLA (0) or APV_SYNTH_FIR (1)");
    h->synthesis = mode;
    return APV_OK;
}

int apv_stream_set_evaluation(apv_handle* h, int32_t Pv, int32_t Mv, const double* h_rvA, const double* h_rvB, int32_t n_ranks,
                              const int32_t* ranks) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_evaluation: the stream is initialised (its buffers are allocated there)");
    if (!h_rvA || !h_rvB || !ranks) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_evaluation: null argument");
    if (Pv < 1 || Mv < 1 || Mv > 16 * 65535) return apv_fail(h, APV_ERR_ARG, "evaluation: Pv and Mv must be at least 1 (Mv at most 1048560)");
    if (!apv_eval_pressure_fits(Pv))
        return apv_fail(h, APV_ERR_ARG, "evaluation: one loudspeaker's window of Pv - 1 + 16 float64 samples does not fit 160 KB of LDS (Pv <= 20465)");
    if (n_ranks < 1 || (size_t)n_ranks > h->rank_list.size()) return apv_fail(h, APV_ERR_ARG, "evaluation: between 1 and the handle's number of ranks");
    for (int i = 0; i < n_ranks; ++i) {
        if (i && ranks[i] <= ranks[i - 1]) return apv_fail(h, APV_ERR_ARG, "evaluation: the ranks must be strictly ascending");
        if (std::find(h->rank_list.begin(), h->rank_list.end(), ranks[i]) == h->rank_list.end())
            return apv_fail(h, APV_ERR_ARG, "evaluation: a rank that is not in the handle's rank list");
    }
    const size_t n = (size_t)Pv * h->cfg.n_srcs * Mv;
    h->eval_rv[0].assign(h_rvA, h_rvA + n);
    h->eval_rv[1].assign(h_rvB, h_rvB + n);
    h->eval_ranks.assign(ranks, ranks + n_ranks);
    h->eval_Pv = Pv;
    h->eval_Mv = Mv;
    return APV_OK;
}

int apv_stream_set_evaluation_spectra(apv_handle* h, int32_t on) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_evaluation_spectra: the stream is initialised (its buffers are allocated there)");
    if (on != 0 && on != 1) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_evaluation_spectra: 0 (off) or 1 (on)");
    h->eval_spectra = on;
    return APV_OK;
}

int apv_stream_set_evaluation_detectability(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_evaluation_detectability: the stream is initialised (its buffers are allocated there)");
    if (n_channels == 0) {
        h->eval_detect_C = 0;
        h->eval_detect_G2.clear();
        return APV_OK;
    }
    if (n_channels < 0 || n_channels > 512 || !h_G2) return apv_fail(h, APV_ERR_ARG, "evaluation detectability: a table of 1..512 channels");
    if (!std::isfinite(Cs) || !std::isfinite(Ca) || !std::isfinite(Leff) || !(Ca > 0.0))
        return apv_fail(h, APV_ERR_ARG, "evaluation detectability: Cs, Ca and Leff must be finite, Ca positive");
    const size_t n = (size_t)h->cfg.n_bins * n_channels;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(h_G2[i])) return apv_fail(h, APV_ERR_ARG, "evaluation detectability: the table must be finite");
    h->eval_detect_G2.assign(h_G2, h_G2 + n);
    h->eval_detect_C = n_channels;
    h->eval_detect_Cs = Cs; h->eval_detect_Ca = Ca; h->eval_detect_Leff = Leff;
    return APV_OK;
}

int apv_stream_reset_evaluation(apv_handle* h) {
    if (!h || !h->st || !h->st->ev_on) return apv_fail(h, APV_ERR_ARG, "apv_stream_reset_evaluation: no stream with an evaluation stage");
    apv_stream* s = h->st;
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipMemsetAsync(s->ev_tot, 0, sizeof(double) * (size_t)s->ev_Z * (3 * s->ev_E + 1) * s->ev_Mv, h->stream));
    const size_t hb = (size_t)s->ev_nhist * (s->ev_Pv - 1) * s->L * s->esz;
    for (int b = 0; b < 2 && hb > 0; ++b) SCHK(h, hipMemsetAsync(s->ev_hist[b], 0, hb, h->stream));
    if (s->es_on) {
        SCHK(h, hipMemsetAsync(s->es_tot, 0, sizeof(double) * (size_t)s->ev_Z * (3 * s->ev_E + 1) * s->K * s->ev_Mv, h->stream));
        SCHK(h, hipMemsetAsync(s->es_ring, 0, sizeof(double) * (size_t)s->ev_sets * s->ev_Mv * s->N, h->stream));
    }
    if (s->ed_on) SCHK(h, hipMemsetAsync(s->ed_tot, 0, sizeof(double) * (size_t)s->ev_Z * 6 * s->ev_E * s->ev_Mv, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

int apv_stream_set_stat_forgetting(apv_handle* h, double beta) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_stat_forgetting: the stream is initialised (the accumulator is allocated there)");
    if (!(beta > 0.0 && beta <= 1.0)) return apv_fail(h, APV_ERR_ARG, "statistics forgetting factor: in (0, 1]");
    if (h->stat_hops > 1)
        return apv_fail(h, APV_ERR_ARG, "apv_stream_set_stat_forgetting: a statistics window is set (a window and forgetting exclude each other)");
    h->stat_forgetting = beta;
    return APV_OK;
}

int apv_process_block(apv_handle* h, const float* h_in_A, const float* h_in_B, float* h_out) {
    return process_block_t<float>(h, h_in_A, h_in_B, h_out);
}

int apv_process_block_f64(apv_handle* h, const double* h_in_A, const double* h_in_B, double* h_out) {
    return process_block_t<double>(h, h_in_A, h_in_B, h_out);
}

int apv_process_signal(apv_handle* h, int32_t n_hops, const float* h_in_A, const float* h_in_B, float* h_out) {
    return process_signal_t<float>(h, n_hops, h_in_A, h_in_B, h_out);
}

int apv_process_signal_f64(apv_handle* h, int32_t n_hops, const double* h_in_A, const double* h_in_B, double* h_out) {
    return process_signal_t<double>(h, n_hops, h_in_A, h_in_B, h_out);
}

int apv_stream_is_f64(apv_handle* h) { return (h && h->st) ? h->st->f64 : -1; }

long apv_stream_not_converged(apv_handle* h) {
    if (h && h->st) return h->st->not_converged;
    if (h && h->bb) return apv_bb_not_converged(h);
    return -1;
}

// Per-bin statistics and eigenvectors of the CURRENT hop, recomputed in float64 on demand from the hop's control-point
// spectra (nothing on the per-hop path pays for them).  zone 0: bright A->A, dark A->B, target A; zone 1: B->B, B->A, B.
int apv_stream_get_statistics(apv_handle* h, int32_t zone, double* h_RB, double* h_RD, double* h_r, double* h_U,
                              double* h_lam) {
    if (!h || !h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_init has not been called");
    if (zone != 0 && zone != 1) return apv_fail(h, APV_ERR_ARG, "zone must be 0 (A) or 1 (B)");
    apv_stream* s = h->st;
    if (!(s->zones & (1 << zone))) return apv_fail(h, APV_ERR_STATE, "this zone program does not run (run_A / run_B)");
    SCHK(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int K = s->K, L = s->L, M = s->M;
    const size_t mat = (size_t)K * L * L * 16, vec = (size_t)K * L * 16;
    // the work space is sized by (K, L) alone, which a stream never changes: allocated once, kept until apv_stream_free
    void*& dRB = s->stat_ws[0]; void*& dRD = s->stat_ws[1]; void*& dr = s->stat_ws[2]; void*& dU = s->stat_ws[3];
    void*& dw = s->stat_ws[4]; void*& dl = s->stat_ws[5]; void*& dspill = s->stat_ws[6]; void*& dst = s->stat_ws[7];
    if (!dRB) SCHK(h, s->own.device(&dRB, mat));
    if (!dRD) SCHK(h, s->own.device(&dRD, mat));
    if (!dr) SCHK(h, s->own.device(&dr, vec));
    if (explicit_stats(s)) {
        // the windowed (or forgetting) statistics of the last hop are in device memory: handed out as they are (c64 widened first)
        const size_t nm = (size_t)K * L * L, nv = (size_t)K * L;
        hipMemcpyKind dd = hipMemcpyDeviceToDevice;
        if (s->win_c128) {
            SCHK(h, hipMemcpyAsync(dRB, s->win_RB[zone], mat, dd, st));
            SCHK(h, hipMemcpyAsync(dRD, s->win_RD[zone], mat, dd, st));
            SCHK(h, hipMemcpyAsync(dr, s->win_r[zone], vec, dd, st));
        } else {
            SCHK(h, apv_launch_widen_c64(nm, s->win_RB[zone], dRB, st));
            SCHK(h, apv_launch_widen_c64(nm, s->win_RD[zone], dRD, st));
            SCHK(h, apv_launch_widen_c64(nv, s->win_r[zone], dr, st));
        }
    }
    const void* XB = zone ? s->X[3] : s->X[0];
    const void* XD = zone ? s->X[2] : s->X[1];
    if (!explicit_stats(s) && s->xg > 1) {
        // grouped spectra: the correlation kernel reads bin-major slabs, so the two sets are regrouped into scratch first
        void*& dgb = s->stat_ws[8]; void*& dgd = s->stat_ws[9];
        const size_t sb = (size_t)K * s->C * 2 * s->esz;
        if (!dgb) SCHK(h, s->own.device(&dgb, sb));
        if (!dgd) SCHK(h, s->own.device(&dgd, sb));
        SCHK(h, apv_launch_ungroup_spectra(s->f64, K, s->C, s->xg, XB, dgb, st));
        SCHK(h, apv_launch_ungroup_spectra(s->f64, K, s->C, s->xg, XD, dgd, st));
        XB = dgb;
        XD = dgd;
    }
    hipError_t e = explicit_stats(s) ? hipSuccess
                 : L > APV_MAX_N ? apv_launch_corr128(K, M, L, s->f64, XB, XD, s->tspec[zone], (double2*)dRB, (double2*)dRD, (double2*)dr, st)
                 : s->f64 ? apv_launch_corr_c128(K, M, L, (const double2*)XB, (const double2*)XD, (const double2*)s->tspec[zone],
                                                 (double2*)dRB, (double2*)dRD, (double2*)dr, st)
                          : apv_launch_corr(APV_F64, K, M, L, (const float2*)XB, (const float2*)XD, (const float2*)s->tspec[zone], dRB, dRD,
                                            dr, st);
    if (e != hipSuccess) return apv_fail(h, APV_ERR_HIP, std::string("statistics: ") + hipGetErrorString(e));
    if (h_U || h_lam) {
        if (!dU) SCHK(h, s->own.device(&dU, mat));
        if (!dw) SCHK(h, s->own.device(&dw, vec));
        if (!dl) SCHK(h, s->own.device(&dl, (size_t)K * L * 8));
        if (!dst) SCHK(h, s->own.device(&dst, (size_t)K * 4));
        GevdParams p = apv_base_params(h);
        p.span = SpanParams{};     // U and lambda do not depend on the span, and its outputs stay those of the last hop
        const size_t sb = apv_gevd_spill_bytes(L, K, APV_F64, p.reg_mode, p.reg_bright, p.sweep_tol2, 1);
        if (sb > s->stat_spill_bytes) {
            s->own.release(dspill);
            s->stat_spill_bytes = 0;
            SCHK(h, s->own.device(&dspill, sb));
            s->stat_spill_bytes = sb;
        }
        p.nV = 1; p.ranks[0] = 1; p.out_c128 = 1; p.n_zones = 1;
        // a window of fewer than L rows (win_fill_host hops are in it now): not for kernels_gevd64.hip, see win_low_rank
        p.no_gevd64 = s->fg_beta > 0.0 ? s->fg_no_gevd64 : (s->win_T > 1 ? (long)s->win_fill_host * M < L : M < L);
        p.RB = dRB; p.RD = dRD; p.r = dr; p.w = dw; p.lam = dl; p.status = (int32_t*)dst; p.U = dU; p.Lspill = dspill;
        std::string why;
        e = apv_launch_gevd(p, APV_F64, false, st, &why);
        if (e != hipSuccess) return launch_fail(h, e, why);
    }
    if (h_RB) SCHK(h, hipMemcpyAsync(h_RB, dRB, mat, hipMemcpyDeviceToHost, st));
    if (h_RD) SCHK(h, hipMemcpyAsync(h_RD, dRD, mat, hipMemcpyDeviceToHost, st));
    if (h_r) SCHK(h, hipMemcpyAsync(h_r, dr, vec, hipMemcpyDeviceToHost, st));
    if (h_U) SCHK(h, hipMemcpyAsync(h_U, dU, mat, hipMemcpyDeviceToHost, st));
    if (h_lam) SCHK(h, hipMemcpyAsync(h_lam, dl, (size_t)K * L * 8, hipMemcpyDeviceToHost, st));
    SCHK(h, hipStreamSynchronize(st));
    return APV_OK;
}

// Enable (n_channels > 0) or disable (0) the perceptual weighting.  h_G2 [K][n_channels]: squared
// outer/middle-ear x gammatone responses (perceptualModel.m:52-54); Cs, Ca, Leff: perceptualModel.m:57, 114-115;
// normalisation 0: unit vector over the K bins (apvast.py:322-324), 1: over the full symmetric curve
// (perceptualModel.m:177-190).                                        replaces apvast.py:313-324 / apVast.m:386-408
int apv_stream_set_perceptual(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff,
                              int32_t normalisation) {
    if (!h || !h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_init has not been called");
    apv_stream* s = h->st;
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipStreamSynchronize(h->stream));
    drop_hop_graphs(s);          // the captured launch sequences depend on whether the weighting is on
    if (n_channels <= 0) {
        s->nch = 0;
        s->xg = s->xg_default;
        return APV_OK;
    }
    if (!h_G2 || n_channels > 512 || (normalisation != 0 && normalisation != 1)) return apv_fail(h, APV_ERR_ARG, "bad perceptual tables");
    s->xg = 1;                   // the weighting's kernels scale bin-major spectra
    const int K = s->K;
    s->own.release(s->G2);
    s->own.release(s->G2T);
    for (int z = 0; z < 2; ++z) s->own.release(s->Wgt[z]);
    std::vector<double> gt((size_t)n_channels * K);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < n_channels; ++i) gt[(size_t)i * K + k] = h_G2[(size_t)k * n_channels + i];
    SCHK(h, s->own.device(&s->G2, sizeof(double) * (size_t)K * n_channels));
    SCHK(h, s->own.device(&s->G2T, sizeof(double) * (size_t)K * n_channels));
    for (int z = 0; z < 2; ++z) SCHK(h, s->own.device(&s->Wgt[z], s->esz * (size_t)K * s->M));
    // on the handle's stream, like every other upload of this file (a null-stream copy is not ordered with it)
    SCHK(h, hipMemcpyAsync(s->G2, h_G2, sizeof(double) * (size_t)K * n_channels, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipMemcpyAsync(s->G2T, gt.data(), sizeof(double) * gt.size(), hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));               // gt goes out of scope; h_G2 is the caller's
    s->nch = n_channels; s->Cs = Cs; s->Ca = Ca; s->Leff = Leff; s->norm_mode = normalisation;
    return APV_OK;
}

// New responses between two hops.  NULL = that response is unchanged; targets are (P, M).  Every tail is formed from the banks as
// they are before this call; the next hops add them to K1's output (kernels_live.hip).     replaces `ap.rir_A = ...` between two
// calls of process_input_buffers, read by lfilter(..., zi=state) at apvast.py:167-193
int apv_stream_set_rirs(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B, const double* h_trir_A,
                        const double* h_trir_B) {
    if (!h || !h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_init has not been called");
    apv_stream* s = h->st;
    if (rir_len != s->P) return apv_fail(h, APV_ERR_ARG, "rir_len must equal the stream's response length");
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipStreamSynchronize(h->stream));
    const double* nw[4] = {h_rir_A, h_rir_B, h_trir_A, h_trir_B};
    if (!nw[0] && !nw[1] && !nw[2] && !nw[3]) return APV_OK;
    FirLiveBanks b{};
    b.P = s->P; b.H = s->H; b.L = s->L; b.M = s->M; b.f64 = s->f64;
    for (int z = 0; z < 2; ++z) {
        b.rir[z] = s->rir[z];
        b.trir[z] = s->trir[z];
        // the current history ends with the newest sample: [keep samples before the last hop | the last hop]
        b.hist_tail[z] = (const char*)s->xhist[s->cur][z] + (size_t)(s->keep + s->H - (s->P - 1)) * s->esz;
    }
    int rc = apv_live_update(h, s->live, b, nw, h->stream);
    if (rc != APV_OK) return rc;
    if (s->fir_F > 0) {
        // the fast-convolution K1 reads spectra of the banks: recomputed in place from the new ones
        if (!s->live_cm) SCHK(h, s->own.device(&s->live_cm, s->esz * (size_t)s->P * s->C));
        for (int k = 0; k < 4; ++k) {
            if (!nw[k]) continue;
            const int n_ch = k < 2 ? s->C : s->M;
            SCHK(h, apv_launch_bank_transpose(s->f64, s->P, n_ch, k < 2 ? s->rir[k] : s->trir[k - 2], s->live_cm, h->stream));
            if ((rc = bank_spectra(h, s->live_cm, n_ch, k < 2 ? s->rirspec[k] : s->trirspec[k - 2]))) return rc;
        }
    }
    SCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

// ---- the per-bin span (include/apvast_hip.h, gevd_span.h) ----
// mu_eff = cfg.mu * profile, uploaded on the handle's stream
static int span_upload_mu(apv_handle* h) {
    apv_handle::Span& sp = h->span;
    std::vector<double> eff(sp.profile.size());
    for (size_t i = 0; i < eff.size(); ++i) eff[i] = h->cfg.mu * sp.profile[i];
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipMemcpyAsync(sp.d_mu_eff, eff.data(), sizeof(double) * eff.size(), hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));               // eff goes out of scope
    return APV_OK;
}

// mu of the next hop on (either stream mode).  The per-hop graphs of the subband stream hold it by value: they are captured again.
//                                                         replaces `ap.mu = ...`, read at apvast.py:161, 406-414
int apv_set_mu(apv_handle* h, double mu) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    if (!std::isfinite(mu)) return apv_fail(h, APV_ERR_ARG, "mu must be finite");
    if (h->st) {
        SCHK(h, hipSetDevice(h->device));
        SCHK(h, hipStreamSynchronize(h->stream));
        drop_hop_graphs(h->st);
    }
    h->cfg.mu = mu;
    // a span with a mu profile: the kernels read mu * profile from a table, not the launch's mu
    if (h->span.on && h->span.has_mu) return span_upload_mu(h);
    return APV_OK;
}

int apv_set_span(apv_handle* h, const double* h_mu_profile, const int32_t* h_rank_cap, double contrast_floor) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    apv_handle::Span& sp = h->span;
    const size_t K = (size_t)h->cfg.n_bins, L = (size_t)h->cfg.n_srcs, n = 2 * K;
    const bool has_mu = h_mu_profile != nullptr, has_cap = h_rank_cap != nullptr, has_floor = contrast_floor != 0.0;
    // everything is checked before anything changes
    if (!std::isfinite(contrast_floor) || contrast_floor < 0.0) return apv_fail(h, APV_ERR_ARG, "apv_set_span: the contrast floor must be finite and >= 0");
    if (!has_mu && !has_cap && !has_floor) return apv_fail(h, APV_ERR_ARG, "apv_set_span: no part given");
    if (sp.on) {
        if (has_mu != sp.has_mu || has_cap != sp.has_cap || has_floor != sp.has_floor)
            return apv_fail(h, APV_ERR_ARG, "apv_set_span: the first call fixed which parts the span has; a part cannot be added or removed");
    } else {
        if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_set_span: the stream is initialised (a span is given before apv_stream_init)");
        if (h->bb) return apv_fail(h, APV_ERR_ARG, "apv_set_span: the span is a subband feature; this handle runs the broadband stream");
        if (h->n_lanes > 1) return apv_fail(h, APV_ERR_ARG, "apv_set_span: not with two update streams (the span's outputs are one buffer)");
    }
    for (size_t i = 0; has_mu && i < n; ++i)
        if (!std::isfinite(h_mu_profile[i]) || h_mu_profile[i] < 0.0) return apv_fail(h, APV_ERR_ARG, "apv_set_span: the mu profile must be finite and >= 0");
    for (size_t i = 0; has_cap && i < n; ++i)
        if (h_rank_cap[i] < 1 || h_rank_cap[i] > (int32_t)L) return apv_fail(h, APV_ERR_ARG, "apv_set_span: rank cap out of 1..L");
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipStreamSynchronize(h->stream));
    if (!sp.on) {
        const size_t nn = n ? n : 1, nc = nn * (L ? L : 1);
        // all four buffers or none: a failure frees what the call had allocated, so that a second first call starts clean
        hipError_t e = hipSuccess;
        if (has_mu) e = hipMalloc((void**)&sp.d_mu_eff, sizeof(double) * nn);
        if (e == hipSuccess && has_cap) e = hipMalloc((void**)&sp.d_cap, sizeof(int32_t) * nn);
        if (e == hipSuccess) e = hipMalloc((void**)&sp.d_rank, sizeof(int32_t) * nn);
        if (e == hipSuccess) e = hipMemsetAsync(sp.d_rank, 0, sizeof(int32_t) * nn, h->stream);
        if (e == hipSuccess && has_floor) e = hipMalloc((void**)&sp.d_contrast, sizeof(double) * nc);
        if (e == hipSuccess && has_floor) e = hipMemsetAsync(sp.d_contrast, 0, sizeof(double) * nc, h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            void** bufs[] = {(void**)&sp.d_mu_eff, (void**)&sp.d_cap, (void**)&sp.d_rank, (void**)&sp.d_contrast};
            for (void** b : bufs) {
                if (*b) (void)hipFree(*b);
                *b = nullptr;
            }
            return apv_fail(h, APV_ERR_HIP, std::string("apv_set_span: ") + hipGetErrorString(e));
        }
        sp.has_mu = has_mu; sp.has_cap = has_cap; sp.has_floor = has_floor;
        sp.on = true;
    }
    if (has_cap) {
        SCHK(h, hipMemcpyAsync(sp.d_cap, h_rank_cap, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));           // h_rank_cap is the caller's
    }
    if (has_floor && contrast_floor != sp.phi) {
        if (h->st) drop_hop_graphs(h->st);                  // the per-hop graphs hold phi by value, like mu
        sp.phi = contrast_floor;
    }
    if (has_mu) {
        sp.profile.assign(h_mu_profile, h_mu_profile + n);
        return span_upload_mu(h);
    }
    return APV_OK;
}

int apv_get_span(apv_handle* h, int32_t zone, int32_t* h_rank, double* h_contrast) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    const apv_handle::Span& sp = h->span;
    if (!sp.on) return apv_fail(h, APV_ERR_ARG, "apv_get_span: the handle has no span (apv_set_span)");
    if (zone != 0 && zone != 1) return apv_fail(h, APV_ERR_ARG, "apv_get_span: zone must be 0 or 1");
    if (h_contrast && !sp.has_floor) return apv_fail(h, APV_ERR_ARG, "apv_get_span: the contrast curve is written only with a contrast floor");
    const size_t K = (size_t)h->cfg.n_bins, L = (size_t)h->cfg.n_srcs;
    SCHK(h, hipSetDevice(h->device));
    if (h_rank) SCHK(h, hipMemcpyAsync(h_rank, sp.d_rank + zone * K, sizeof(int32_t) * K, hipMemcpyDeviceToHost, h->stream));
    if (h_contrast) SCHK(h, hipMemcpyAsync(h_contrast, sp.d_contrast + zone * K * L, sizeof(double) * K * L, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

// ---- the per-bin array-effort limit (include/apvast_hip.h, kernels_effort.hip) ----
int apv_stream_set_effort_limit(apv_handle* h, const double* h_limit) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    if (!h_limit) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_effort_limit: null table");
    apv_handle::Effort& ef = h->effort;
    const size_t K = (size_t)h->cfg.n_bins, L = (size_t)h->cfg.n_srcs, n = 2 * K;
    // everything is checked before anything changes
    if (h->bb) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_effort_limit: the effort limit is a subband feature; this handle runs the broadband stream");
    if (!ef.on && h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_effort_limit: the stream is initialised (the first limit is given before apv_stream_init)");
    for (size_t i = 0; i < n; ++i)
        if (!(h_limit[i] > 0.0)) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_effort_limit: a limit must be > 0 (+inf: no limit), not NaN");
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipStreamSynchronize(h->stream));
    if (!ef.on) {
        // the table and the outputs, all or none: a failure frees what the call had allocated.  The effort curve has room for
        // every rank list the handle can take (n_ranks <= n_srcs)
        ApvOwned* own = new ApvOwned;
        double *lim = nullptr, *eff = nullptr, *gain = nullptr;
        int32_t* src = nullptr;
        hipError_t e = own->device(&lim, sizeof(double) * (n ? n : 1));
        if (e == hipSuccess) e = own->zeroed(&eff, n * (L ? L : 1), sizeof(double), h->stream);
        if (e == hipSuccess) e = own->device(&src, sizeof(int32_t) * (n ? n : 1));
        if (e == hipSuccess) e = hipMemsetAsync(src, 0xff, sizeof(int32_t) * (n ? n : 1), h->stream);     // -1: nothing yet
        if (e == hipSuccess) e = own->zeroed(&gain, n, sizeof(double), h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            delete own;
            return apv_fail(h, APV_ERR_HIP, std::string("apv_stream_set_effort_limit: ") + hipGetErrorString(e));
        }
        ef.own = own; ef.d_limit = lim; ef.d_effort = eff; ef.d_src = src; ef.d_gain = gain;
        ef.on = true;
    }
    // the hop graphs hold the table's address, not its values: no new capture
    SCHK(h, hipMemcpyAsync(ef.d_limit, h_limit, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));               // h_limit is the caller's
    return APV_OK;
}

int apv_get_effort(apv_handle* h, int32_t zone, double* h_effort, int32_t* h_rank, double* h_gain) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    const apv_handle::Effort& ef = h->effort;
    if (!ef.on) return apv_fail(h, APV_ERR_ARG, "apv_get_effort: the handle has no effort limit (apv_stream_set_effort_limit)");
    if (zone != 0 && zone != 1) return apv_fail(h, APV_ERR_ARG, "apv_get_effort: zone must be 0 or 1");
    const size_t K = (size_t)h->cfg.n_bins, nV = (size_t)h->cfg.n_ranks;
    SCHK(h, hipSetDevice(h->device));
    if (h_effort) SCHK(h, hipMemcpyAsync(h_effort, ef.d_effort + zone * K * nV, sizeof(double) * K * nV, hipMemcpyDeviceToHost, h->stream));
    if (h_rank) SCHK(h, hipMemcpyAsync(h_rank, ef.d_src + zone * K, sizeof(int32_t) * K, hipMemcpyDeviceToHost, h->stream));
    if (h_gain) SCHK(h, hipMemcpyAsync(h_gain, ef.d_gain + zone * K, sizeof(double) * K, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    // the kernel leaves the source slot of the top slot (-1: its effort was not finite, or no hop has run); the caller gets that
    // slot's rank
    if (h_rank)
        for (size_t k = 0; k < K; ++k) h_rank[k] = (h_rank[k] < 0 || (size_t)h_rank[k] >= nV) ? 0 : h->rank_list[(size_t)h_rank[k]];
    return APV_OK;
}

// ---- the rank choice by the contrast at validation microphones (include/apvast_hip.h, kernels_valspan.hip) ----
int apv_stream_set_validation_span(apv_handle* h, const void* h_G_A, const void* h_G_B, const double* h_floor) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    if (!h_floor) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: null floor table");
    apv_handle::ValSpan& vs = h->valspan;
    const size_t K = (size_t)h->cfg.n_bins, L = (size_t)h->cfg.n_srcs, n = 2 * K;
    // everything is checked before anything changes
    if (h->bb) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: the validation span is a subband feature; this handle runs the broadband stream");
    if (!vs.on) {
        if (h->st) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: the stream is initialised (the first call comes before apv_stream_init)");
        if (h->eval_Pv <= 0) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: the first call comes after apv_stream_set_evaluation (it sizes the transfer functions)");
        if (!h_G_A || !h_G_B) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: the first call needs both transfer functions");
        if (L > (size_t)APV_VALSPAN_MAX_SLOTS) return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: at most 128 loudspeakers");
    } else if ((h_G_A != nullptr) != (h_G_B != nullptr)) {
        return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: both transfer functions or neither");
    }
    for (size_t i = 0; i < n; ++i)
        if (!(h_floor[i] >= 0.0) || !std::isfinite(h_floor[i]))
            return apv_fail(h, APV_ERR_ARG, "apv_stream_set_validation_span: a floor must be finite and >= 0 (0: no floor), not NaN");
    SCHK(h, hipSetDevice(h->device));
    SCHK(h, hipStreamSynchronize(h->stream));
    const size_t Mv = vs.on ? (size_t)vs.Mv : (size_t)h->eval_Mv, gbytes = 16 * K * Mv * L;
    if (!vs.on) {
        // the banks, the table and the outputs, all or none: a failure frees what the call had allocated.  The outputs have room
        // for every rank list the handle can take (n_ranks <= n_srcs)
        ApvOwned* own = new ApvOwned;
        void *gA = nullptr, *gB = nullptr;
        double *phi = nullptr, *bright = nullptr, *dark = nullptr;
        int32_t* src = nullptr;
        const size_t no = n * (L ? L : 1);
        hipError_t e = own->device(&gA, gbytes ? gbytes : 1);
        if (e == hipSuccess) e = own->device(&gB, gbytes ? gbytes : 1);
        if (e == hipSuccess) e = own->device(&phi, sizeof(double) * (n ? n : 1));
        if (e == hipSuccess) e = own->zeroed(&bright, no, sizeof(double), h->stream);
        if (e == hipSuccess) e = own->zeroed(&dark, no, sizeof(double), h->stream);
        if (e == hipSuccess) e = own->device(&src, sizeof(int32_t) * (no ? no : 1));
        if (e == hipSuccess) e = hipMemsetAsync(src, 0xff, sizeof(int32_t) * (no ? no : 1), h->stream);     // -1: nothing yet
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            delete own;
            return apv_fail(h, APV_ERR_HIP, std::string("apv_stream_set_validation_span: ") + hipGetErrorString(e));
        }
        vs.own = own; vs.d_G[0] = gA; vs.d_G[1] = gB; vs.d_phi = phi; vs.d_bright = bright; vs.d_dark = dark; vs.d_src = src;
        vs.Mv = (int)Mv;
        vs.on = true;
    }
    // the hop graphs hold the addresses of the banks and the table, not their values: no new capture
    if (h_G_A) {
        SCHK(h, hipMemcpyAsync(vs.d_G[0], h_G_A, gbytes, hipMemcpyHostToDevice, h->stream));
        SCHK(h, hipMemcpyAsync(vs.d_G[1], h_G_B, gbytes, hipMemcpyHostToDevice, h->stream));
    }
    SCHK(h, hipMemcpyAsync(vs.d_phi, h_floor, sizeof(double) * n, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));               // the arrays are the caller's
    return APV_OK;
}

int apv_get_validation_span(apv_handle* h, int32_t zone, int32_t what, void* h_dst) {
    if (!h) return apv_fail(h, APV_ERR_ARG, "null handle");
    const apv_handle::ValSpan& vs = h->valspan;
    if (!vs.on) return apv_fail(h, APV_ERR_ARG, "apv_get_validation_span: the handle has no validation span (apv_stream_set_validation_span)");
    if (zone != 0 && zone != 1) return apv_fail(h, APV_ERR_ARG, "apv_get_validation_span: zone must be 0 or 1");
    if (what < APV_VALSPAN_BRIGHT || what > APV_VALSPAN_RANK) return apv_fail(h, APV_ERR_ARG, "apv_get_validation_span: what must be one of APV_VALSPAN_*");
    if (!h_dst) return apv_fail(h, APV_ERR_ARG, "apv_get_validation_span: null destination");
    const size_t K = (size_t)h->cfg.n_bins, nV = (size_t)h->cfg.n_ranks, o = (size_t)zone * K * nV;
    SCHK(h, hipSetDevice(h->device));
    if (what == APV_VALSPAN_BRIGHT || what == APV_VALSPAN_DARK) {
        const double* src = (what == APV_VALSPAN_BRIGHT ? vs.d_bright : vs.d_dark) + o;
        SCHK(h, hipMemcpyAsync(h_dst, src, sizeof(double) * K * nV, hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
        return APV_OK;
    }
    if (what == APV_VALSPAN_SOURCE) {
        SCHK(h, hipMemcpyAsync(h_dst, vs.d_src + o, sizeof(int32_t) * K * nV, hipMemcpyDeviceToHost, h->stream));
        SCHK(h, hipStreamSynchronize(h->stream));
        return APV_OK;
    }
    // the rank of the top slot's source: the top column of the sources, then the slot's entry of the rank list
    int32_t* rank = static_cast<int32_t*>(h_dst);
    std::vector<int32_t> src(K * nV);
    SCHK(h, hipMemcpyAsync(src.data(), vs.d_src + o, sizeof(int32_t) * K * nV, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    for (size_t k = 0; k < K; ++k) {
        const int32_t t = src[k * nV + nV - 1];
        rank[k] = (t < 0 || (size_t)t >= nV) ? 0 : h->rank_list[(size_t)t];
    }
    return APV_OK;
}

}  // extern "C"
