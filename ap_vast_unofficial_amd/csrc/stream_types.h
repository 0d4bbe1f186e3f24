// The subband stream's state (struct apv_stream) and the few helpers its translation units share: stream.hip (set-up, hops,
// whole signals, setters) and stream_state.hip (the named state arrays).  Private to those two files.
#pragma once
#include "apv_internal.h"
#include "apv_owned.h"

constexpr int CK_NB = 4;      // back streams of the chunked whole-signal path
constexpr int CK_NS = 3;      // pinned staging slots (chunks) of that path

// A measuring aid around one launch of the hop (statistics, projection, FIR synthesis): the events exist only where the stage's
// environment switch is set, and run_hop reads them after every hop.
struct StageTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};      // recorded in front of and behind the launch
    double ms[2] = {0.0, 0.0};                  // {sum of its times in ms, hops timed}
    hipError_t read() {
        if (!ev[0]) return hipSuccess;
        float t = 0.f;
        const hipError_t e = hipEventElapsedTime(&t, ev[0], ev[1]);
        if (e == hipSuccess) { ms[0] += t; ms[1] += 1.0; }
        return e;
    }
};

struct apv_stream {
    int N, H, K, L, M, C, P, nV, zones, pad;
    int f64;                      // precision of the whole front-end: RIRs, rings, spectra, overlap buffers, outputs
    size_t esz;                   // bytes per real sample (4 | 8); a complex spectrum element is 2 esz
    int ring_off;                 // physical index of logical sample 0 in every ring
    int cur;                      // which input-history buffer is current
    int n_out;                    // synthesis channels: zones*nV*L filtered + 2*L target
    int out_group;                // cfg.out_layout = 1: L (hops are emitted [n_out / L][H][L]); 0 = channel-major [n_out][H]
    void* rir[2];                 // [P][C]  zone A, zone B
    void* trir[2];                // [P][M]  target RIRs (reference loudspeaker, delayed)
    void* xhist[2][2];            // [buf][signal][keep+H+pad]
    void* resp[4];                // [C][N] rings: A->A, A->B, B->A, B->B
    void* tresp[2];               // [M][N] rings: target A, target B
    void* inblk;                  // [2][N] rings: input blocks
    void* X[4];                   // control-point spectra: bin-major [K][C], or grouped [Kp / xg][C][xg] (see xg); Kp C elements each
    int xg, xg_default;           // bins per group of the spectra layout (1 = bin-major).  4 where the joint diagonalisation that will
                                  // run reads groups (float64 front-end, order 16, apv_gevd_reads_groups) and no perceptual weighting
                                  // is on (its kernels scale bin-major spectra): a transform then fills 64-byte lines
    int Kp;                       // K rounded up to a multiple of 8: bins a spectra set is allocated for
    void* tspec[2];               // [K][M]
    void* inspec;                 // [2][K]
    void* w[2];                   // [K][nV][L] per zone
    void* lam[2];                 // [K][L]
    int32_t* status[2];           // [K]
    void* tgt;                    // [L][K] target filter spectra (shared by A_t and B_t, apvast.py:389-390)
    void* outspec;                // [n_out][K]
    void* outov;                  // [n_out][N]
    void* out;                    // [n_out][H] samples, then the [2][K] status words of the hop: one copy back
    // perceptual weighting (off when nch == 0)
    int nch, norm_mode;
    double Cs, Ca, Leff;
    double* G2;                   // [K][nch]
    double* G2T;                  // [nch][K]
    void* Wgt[2];                 // [K][M] per zone
    // pinned staging + one captured hipGraph per phase of the (ring offset, history buffer) cycle
    void* pin_in;                 // [2][H]
    void* pin_out;                // [n_out][H] samples + [2][K] status words
    int period;                   // hops after which (ring_off, cur) repeat; 0 = graphs off
    // whole-signal path (apv_process_signal): a second set of the hop's spectra, a second stream and four events, so
    // that the front half (FIR + analysis) of hop h+1 runs beside the back half (GEVD + synthesis) of hop h
    void* X1[4];                  // like X, tspec, inspec: hops alternate between the two sets
    void* tspec1[2];
    void* inspec1;
    hipStream_t front;            // front-half stream; the back half stays on the handle's stream
    hipEvent_t ev_front[2];       // set p filled by the front half
    hipEvent_t ev_back[2];        // set p released by the back half
    hipEvent_t ev_chunk[2];       // chunk c & 1 of the pinned staging complete
    // ... and a tail stream with second output-spectra and result buffers: synthesis and copy back of hop h run beside
    // the joint diagonalisation of hop h+1 instead of in front of it
    void* outspec1;               // like outspec, out; hops alternate between the two
    void* out1;
    hipStream_t tail;
    hipEvent_t ev_copied[2];      // result buffer b copied to the host
    void* sig_in;                 // pinned [2][chunk][2][H]
    void* sig_out;                // pinned [2][chunk] hop results (samples [n_out][H] + status words [2][K] each)
    int sig_chunk;                // hops per half of the pinned staging
    // K1 by fast convolution (fir_F > 0): spectra of the zero-padded impulse responses and of the two input histories
    // of the hop, in the front-end precision
    int fir_F;                    // segment length, 0 = direct form
    int fir_np;                   // partitions of the uniformly partitioned form (responses too long for one segment), else 1
    int keep;                     // input samples the histories keep in front of the hop: P - 1, or fir_np H when partitioned
    void* rirspec[2];             // [fir_np][C][fir_F/2 + 1] complex, zone A, zone B
    void* trirspec[2];            // [fir_np][M][fir_F/2 + 1]
    void* xspec;                  // [fir_np][2][fir_F/2 + 1]
    void* xspec_chunk;            // [sig_chunk][2][fir_F/2 + 1]: whole-signal path, the spectra of a staged chunk in one launch
    long hop;                     // hops processed
    long not_converged;           // hops in which some bin hit the sweep cap (status 2)
    // chunked whole-signal path (process_signal_chunked_t): the FRONT half of a whole chunk of hops is three launches (input side,
    // K1, analysis) into linear buffers and one spectra set per hop; the back halves of consecutive hops alternate between two
    // streams with their own filters, output spectra and result buffers.  Everything is allocated at the path's first call.
    int ck_RL;                    // row length of the linear buffers: N - H + sig_chunk H (0 = not set up)
    void* ck_resp[2][4];          // [chunk parity][path]: [C][RL]
    void* ck_tresp[2][2];         // [M][RL]
    void* ck_in[2];               // [2][RL]
    void* ck_X[4];                // [2 sig_chunk][K][C]: set (parity, i) = parity sig_chunk + i
    void* ck_tspec[2];            // [2 sig_chunk][K][M]
    void* ck_inspec;              // [2 sig_chunk][2][K]
    void* ck_w[CK_NB - 1][2];     // [K][nV][L] per zone: filters of back streams 1 ... (back stream 0 uses w, lam)
    void* ck_lam[CK_NB - 1][2];
    void* ck_wall[2];             // [sig_chunk][K][nV][L] per zone: the filters of every hop of a chunk whose joint diagonalisations are ONE launch
    void* ck_lamall[2];           // [sig_chunk][K][L]
    void* ck_spill[CK_NB - 1];    // per-bin scratch of the joint diagonalisation (orders 33..64) for back streams 1 ...: two hops' workgroups for
                                  // the same bin run at once, each parks its state in its own stream's slot (back stream 0 uses d_Lspill)
    hipStream_t ck_back[CK_NB - 1];
    void* ck_pin_in;              // pinned [CK_NS][sig_chunk][2][H]: the host stages chunk c + 1 while chunks c - 1 and c are in flight
    void* ck_pin_out;             // pinned [CK_NS][sig_chunk] hop results
    hipEvent_t ck_done[CK_NS];    // the chunk in staging slot q has been copied back
    void* ck_out;                 // [2 sig_chunk] hop results (samples [n_out][H] + status words [2][K]): one slot per hop of two chunks
    void* ck_ospec;               // [2 sig_chunk][n_out][K] output spectra, likewise
    hipEvent_t ck_backdone[2][CK_NB]; // [chunk parity][back stream]: that stream has read the parity's spectra sets for the last time
    hipEvent_t ck_k3[CK_NB];      // [back stream]: output spectra written (the tail stream starts the synthesis there)
    // work space of apv_stream_get_statistics (R_B, R_D, r, U, w, lam, spill, status), allocated at its first call and kept
    void* stat_ws[10];
    size_t stat_spill_bytes;
    // responses reassigned between hops (apv_stream_set_rirs): the tails still to be added to K1's output, and a channel-major
    // copy of one bank for its fast-convolution spectra; allocated at the first update
    FirLive live;
    void* live_cm;
    // statistics window (apv_stream_set_stat_hops, kernels_statwin.hip); win_T = 1: off, the fused single-block update runs
    int win_T;                    // hops in the window
    int win_c128;                 // ring and window sums are c128 (float64 joint diagonalisation), else c64
    void* win_ring[2];            // per zone program: [win_T][K][2 L^2 + L] Gram matrices of the last hops
    void* win_RB[2];              // per zone program: the window sums the joint diagonalisation reads, [K][L][L], [K][L][L], [K][L]
    void* win_RD[2];
    void* win_r[2];
    int32_t* win_ctr;             // device words {head, fill}: read by the hop's statistics kernel, advanced behind it
    int win_fill_host;            // the host's copy of fill (hops in the window before the next one), kept in step by run_hop and by
                                  // the state "stat_window_fill".  Only win_low_rank reads it (which KERNEL solves an order-64 hop):
                                  // the ring position itself never enters a launch from the host
    // exponentially forgetting statistics (apv_stream_set_stat_forgetting): R <- fg_beta R + G per hop.  win_T stays 1; the
    // accumulator is the one slot win_ring[z] [K][2 L^2 + L], and win_c128, win_RB / win_RD / win_r, win_tm serve as above
    double fg_beta;               // 0: off
    int fg_no_gevd64;             // GevdParams::no_gevd64 of every hop and of apv_stream_get_statistics: see apv_stream_init
    // filter-length constraint (apv_stream_set_filter_taps, kernels_constrain.hip); taps = 0: off, nothing below exists
    int taps;                     // J
    void* wtaps[2];               // per zone program: [nV][J][L] real, the J taps of the hop's projected filters (precision of w)
    StageTimer cf_tm;             // APV_FILTER_CONSTRAINT_TIMING (tools/bench_filter_constraint.py): the projection
    // FIR synthesis (apv_stream_set_synthesis, kernels_firsynth.hip); fir_synth = 0: off, nothing below exists
    int fir_synth;
    int fs_ref, fs_delay;         // the target paths: column reference_index_A, modeling_delay samples late
    void* fs_taps[2];             // per zone program that runs: [nV][J][L], the taps the next hop fades from (precision of w)
    void* fs_hist[2][2];          // [buf][signal][J - 1]: the newest input samples; buf = cur, like the input histories of K1
    StageTimer fs_tm;             // APV_FIR_SYNTHESIS_TIMING (tools/bench_fir_synthesis.py): the synthesis launch
    // chunked whole-signal path of a constrained stream (process_signal_chunked_t; allocated by chunk_prepare for such a stream only)
    void* ck_taps[2];             // per zone program: [sig_chunk][nV][J][L], the taps of every hop of a chunk (ONE projection launch)
    void* ck_xrow[2][2];          // [chunk parity][signal]: [J - 1 samples before the chunk | sig_chunk H samples of the chunk], FIR synthesis
    hipEvent_t ck_wallfree;       // hop-by-hop regime: the tail stream has read ck_wall / ck_taps of a chunk for the last time
    // evaluation stage (apv_stream_set_evaluation, kernels_streameval.hip); ev_on = 0: off, nothing below exists
    int ev_on;
    int ev_Pv, ev_Mv, ev_E, ev_Z; // response taps, validation microphones, evaluated ranks, zone programs that run
    int ev_sets, ev_nhist;        // pressure sets ev_Z (2 ev_E + 1), evaluated groups ev_Z (ev_E + 1)
    double* ev_rv[2];             // validation responses of zone A, zone B: [Pv][L][Mv]
    int32_t* ev_map;              // [ev_sets][4]: {group of the result buffer, history slot, response bank, 0}
    int32_t* ev_hsrc;             // [ev_nhist]: group of the result buffer each history slot follows
    void* ev_hist[2];             // [buf][ev_nhist][Pv - 1][L]: the newest output samples; buf = cur, like fs_hist
    double* ev_p;                 // [ev_sets][H][Mv]: the pressures of the last hop
    double* ev_tot;               // [ev_Z][3 ev_E + 1][Mv]: the energies summed over the hops
    double* ev_rec;               // [ev_cap] slots of that shape: the energies of each hop of the last call (grow-only)
    unsigned long long* ev_ctl;   // device words {ev_rec, ev_cap, slot counter of parity 0, of parity 1}: see kernels_streameval.hip
    int ev_cap, ev_nrec;          // slots ev_rec holds; hops of the last call (the slots that are valid)
    // per-bin evaluation spectra (apv_stream_set_evaluation_spectra, kernels_evalspec.hip); es_on = 0: off, nothing below exists
    int es_on;
    double* es_ring;              // [ev_sets ev_Mv][N] float64 ring of the pressures, channel-major, at the stream's ring_off
    void* es_spec;                // [K][ev_sets ev_Mv] complex128: the hop's spectra, bin-major scratch
    double* es_tot;               // [ev_Z][3 ev_E + 1][K][ev_Mv]: |P|^2 summed over the hops
    // perceptual detectability of the evaluated pressures (apv_stream_set_evaluation_detectability, kernels_evaldetect.hip), on
    // es_spec; ed_on = 0: off, nothing below exists
    int ed_on;
    int ed_C;                     // channels of the model
    double ed_Cs, ed_Ca, ed_Leff;
    double* ed_G2T;               // [ed_C][K]: the squared channel responses, channel-major
    double* ed_quiet;             // [K]: the curve of a silent masker (read with one zone program), formed once
    double* ed_curves;            // [K][ev_Z ev_Mv]: the hop's squared weighting curves
    double* ed_part;              // [chunks][ev_Z][2 ev_E][ev_Mv]: partial sums of the hop
    double* ed_tot;               // [ev_Z][6 ev_E][ev_Mv]: per program sum, max and count of D > 1 of the error, then of the leak
    double* ed_rec;               // [ed_cap] slots [ev_Z][2 ev_E][ev_Mv]: the values of each hop of the last call (grow-only, like ev_rec)
    unsigned long long* ed_ctl;   // device words {ed_rec, ed_cap, hops of the call so far}: see kernels_evaldetect.hip
    int ed_cap;                   // slots ed_rec holds (ev_nrec of them are valid)
    int32_t sched[2];             // state "signal_schedule": hops of the last whole-signal call {through chunk launches, hop by hop}
    StageTimer win_tm;            // APV_STAT_WINDOW_TIMING (tools/bench_stat_window.py): the statistics launch
    std::vector<hipGraphExec_t> execs;
    std::vector<int32_t> h_status;
    ApvOwned own;                 // every buffer, pinned block, event and stream above: made through it, freed by it
};

#define HIPCHK(h, call, what)                                                            \
    do {                                                                                 \
        hipError_t _e = (call);                                                          \
        if (_e != hipSuccess) return apv_fail(h, APV_ERR_HIP, std::string(what) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define SCHK(h, call) HIPCHK(h, call, #call)

// bytes of a filter coefficient and of an eigenvalue or tap in the precision of the outputs (cfg.out_c128)
inline size_t wsz(const apv_handle* h) { return h->cfg.out_c128 ? 16 : 8; }
inline size_t lsz(const apv_handle* h) { return h->cfg.out_c128 ? 8 : 4; }
