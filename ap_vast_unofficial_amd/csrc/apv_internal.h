// Internal declarations shared by the HIP translation units of libapvast_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/apvast_hip.h"
#include "gevd_span.h"

struct GevdParams {
    int n;            // GEVD order (= L in subband mode)
    int M;            // control points per zone (fused path only)
    int K;            // problems in this launch
    int nV;
    int ranks[APV_MAX_RANKS];
    double mu;
    double reg_dark;
    double reg_bright;
    int reg_mode;
    int max_sweeps;
    int debug_stop;    // profiling aid: return after stage N (1 = correlate, 2 = Cholesky, 3 = whitening); 0 = run everything.  Values above 3:
                       // A/B switches of the diagnostic order-16 (4, 5, 9, 10: kernels_gevd16m.hip) and order-64 (4..8) kernels
    double sweep_tol2; // Jacobi stop threshold on off^2/||C||_F^2 seen during a sweep; 0 = per-dtype default
    int out_c128;
    // fused input: c64, or c128 when x_c128 is set (the float64 streaming front-end)
    int x_c128;
    // fused input in the grouped layout [K / x_group][M n][x_group] (0 or 1: bin-major [K][M][n]); only the order-16 float64 kernel
    // on c128 slabs reads it (kernels_gevd16m.hip), every other kernel refuses a launch with x_group > 1
    int x_group;
    const void* XB;
    const void* XD;
    const void* d;
    // explicit input (complex of the compute dtype), row-major n x n
    const void* RB;
    const void* RD;
    const void* r;
    // outputs
    void* w;          // [K][nV][n]  c64 | c128
    void* lam;        // [K][n]      f32 | f64   (may be null)
    int32_t* status;  // [K]                      (may be null)
    void* U;          // [K][n][n]   complex of compute dtype, sorted columns (may be null)
    void* Lspill;     // [K][n][n]   complex of compute dtype (SPILL instances only)
    // optional second zone program in the same launch (blockIdx.y == 1), fused path only
    int n_zones;
    const void* XB1;
    const void* XD1;
    const void* d1;
    void* w1;
    void* lam1;
    int32_t* status1;
    // streaming: 1 = this launch shares the chip with the transforms of the NEXT chunk of hops, which are the longer chain
    // (chunked whole-signal path): the waves keep the default issue priority instead of raising theirs
    int yield_issue;
    // diagnostic builds only (tools/probes/stage_stamps.py): s_memtime at the stage boundaries, [zones][K][16]; null in normal use
    unsigned long long* stamps;
    // several hops of a chunk in ONE launch (chunked whole-signal path; blockIdx.z = hop): the same K bins for n_hops consecutive spectra
    // sets, byte strides from hop to hop of the slabs (XB, XD and their second-zone twins), the targets, and the three outputs.  Only
    // the order-16 kernels on fused slabs take it (apv_gevd16m_takes_hops); 0 or 1: a single hop, strides unused
    int n_hops;
    size_t hop_X, hop_d, hop_w, hop_lam, hop_status;
    // 1: an order-64 launch goes to the LDS kernel of kernels_gevd.hip, not to kernels_gevd64.hip.  For float64 pencils of rank
    // below n (a statistics window that holds fewer than n rows): loaded with 1e-7 alone, the whitened matrix spans more decades
    // than the float32 sweeps of the order-64 kernel resolve; the LDS kernel's float64 instance sweeps in float64, and its parked
    // factor fits the same scratch slots.  (Explicit float32 statistics never reach kernels_gevd64.hip: nothing to reroute there.)
    // (The fused update of ONE block with fewer control points than loudspeakers, M < n, is such a pencil too: the stream's plain
    // hop and apv_update_dev of a float64 handle, and apv_stream_get_statistics, set the field for it.)
    int no_gevd64;
    // 1: second launch behind kernels_gevd64.hip on the same stream (apv_launch_gevd makes it): a small grid whose workgroups walk
    // the status words and solve the bins left at 2 again, from the same inputs, in float64 throughout
    int only_status2;
    // per-bin mu, per-bin rank cap, contrast floor and their outputs (gevd_span.h); apv_base_params fills it from the handle's span
    // (apv_set_span): z[0] = table row 0 (program A), z[1] = row 1.  A launch whose FIRST zone program is B takes row 1 as z[0]
    // (apv_span_first_zone).  span.on = 0: the launch does what it did before the span existed
    SpanParams span;
};

struct apv_handle {
    apv_config cfg;
    int device;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    // workspaces
    void* d_XB;       // staging for the host-pointer entry points
    void* d_XD;
    void* d_d;
    void* d_w;
    void* d_lam;
    int32_t* d_status;
    void* d_Lspill;
    size_t lspill_bytes;
    void* d_Rscratch;  // [2][K][L][L] + [K][L] c64: MFMA correlation output of the split n in {32, 64} f32 update
    size_t rscratch_bytes;
    unsigned long long* d_stamps;   // apv_debug_set_stamps: stage-stamp buffer of the diagnostic kernel instantiation (caller's)
    struct apv_stream* st;   // streaming state (apv_stream_init), owned
    struct apv_bb* bb;       // broadband streaming state (apv_bb_init), owned
    std::vector<int32_t> rank_list;  // the subband rank list: cfg.ranks, or apv_set_rank_list's (cfg.n_ranks entries, up to n_srcs)
    int stat_hops;                   // apv_stream_set_stat_hops: statistics window of the next apv_stream_init, in hops (<= 1: one block)
    double stat_forgetting;          // apv_stream_set_stat_forgetting: forgetting factor of the next apv_stream_init in (0, 1]; 0: off
    int filter_taps;                 // apv_stream_set_filter_taps: J of the next apv_stream_init's filter-length constraint; 0: off
    int synthesis;                   // apv_stream_set_synthesis: APV_SYNTH_WOLA (0) or APV_SYNTH_FIR of the next apv_stream_init
    // apv_stream_set_evaluation: the evaluation stage of the next apv_stream_init (eval_Pv = 0: off)
    int eval_Pv, eval_Mv;
    std::vector<double> eval_rv[2];  // validation responses of zone A, zone B: [Pv][L][Mv]
    std::vector<int32_t> eval_ranks; // evaluated ranks, ascending, each in rank_list
    int eval_spectra;                // apv_stream_set_evaluation_spectra: per-bin spectra of the evaluation stage (0: off)
    // apv_stream_set_evaluation_detectability: the model tables of the next apv_stream_init's detectability stage (eval_detect_C = 0: off)
    int eval_detect_C;
    std::vector<double> eval_detect_G2;  // [n_bins][eval_detect_C]
    double eval_detect_Cs, eval_detect_Ca, eval_detect_Leff;
    // apv_set_span: which parts exist is fixed by the first call; the tables and outputs are [2][n_bins] (row = zone program)
    struct Span {
        bool on = false, has_mu = false, has_cap = false, has_floor = false;
        double phi = 0.0;
        std::vector<double> profile;     // [2][K] as given: apv_set_mu re-forms mu_eff from it
        double* d_mu_eff = nullptr;      // [2][K]
        int32_t* d_cap = nullptr;        // [2][K]
        int32_t* d_rank = nullptr;       // [2][K]
        double* d_contrast = nullptr;    // [2][K][L], only with a floor
    } span;
    // apv_stream_set_effort_limit: the per-bin array-effort limit of the subband stream's filters (kernels_effort.hip).  The table
    // and the outputs of the last hop are [2][n_bins] (row = zone program); `own` (an ApvOwned, made by the first call) holds them
    struct Effort {
        bool on = false;
        class ApvOwned* own = nullptr;
        double* d_limit = nullptr;       // [2][K], linear, +inf = no limit
        double* d_effort = nullptr;      // [2][K][nV]
        int32_t* d_src = nullptr;        // [2][K]: source slot of the top slot (kernels_effort.hip)
        double* d_gain = nullptr;        // [2][K]
    } effort;
    // apv_stream_set_validation_span: the rank choice by the contrast at the validation microphones (kernels_valspan.hip).  The
    // banks are those of zone A and zone B at the bin centres; the floor and the outputs of the last hop are rows per zone program.
    // `own` (an ApvOwned, made by the first call) holds them
    struct ValSpan {
        bool on = false;
        class ApvOwned* own = nullptr;
        int Mv = 0;                      // eval_Mv of the first call
        void* d_G[2] = {nullptr, nullptr};   // [K][Mv][L] complex128: zone A, zone B
        double* d_phi = nullptr;         // [2][K], linear, 0 = no floor
        double* d_bright = nullptr;      // [2][K][nV]
        double* d_dark = nullptr;        // [2][K][nV]
        int32_t* d_src = nullptr;        // [2][K][nV]: source slot of every slot, -1 = none
    } valspan;
    std::vector<int> bb_rank_list;   // apv_bb_set_rank_list: ranks of the next apv_bb_init (empty = 1..V)
    void* gl_ws;             // workspace + captured sweep graph of apv_gevd_large, owned
    double gl_tol2;          // > 0: stop threshold of apv_gevd_large's sweeps for the next call (the complex path asks for accurate eigenVECTORS)
    int gl_lead_rank;        // > 0: the next apv_gevd_large call needs the leading gl_lead_rank eigenpairs only (kernels_gevd_lead.hip); reset by the call
    int gl_lead_done;        // set by apv_gevd_large: 1 = only the leading columns of U / entries of lambda were written
    void* lead_ws;           // workspace of apv_gevd_lead, owned
    void* comm;       // ncclComm_t
    int comm_rank, comm_world;
    hipStream_t comm_stream;      // the all-gather runs here so that it overlaps the next block's kernels
    hipEvent_t ev_ready;          // compute -> comm: the shard is written
    struct { const void* ptr; hipEvent_t ev; } gather_done[4];   // comm -> compute: shard buffer may be rewritten
    int gather_next;              // slot recycled next when all four track live buffers
    hipEvent_t ev_ag0, ev_ag1;    // timing events around the latest all-gather (comm stream)
    size_t ag_bytes;              // bytes this rank contributed to it
    int32_t* d_bar;               // one device word for apv_comm_barrier
    // update lanes (apv_set_update_streams): consecutive apv_update_dev launches alternate between two streams -- `stream` itself
    // (lane 0) and one more -- so that the tail of one launch (waves of its last round finishing one by one) runs beside the head
    // of the next.  `stream` is also the control stream: copies, timers and the gather's hand-over are ordered against the lanes by events.
    struct UpdateLane {
        hipStream_t s;
        hipEvent_t ev;            // recorded behind the lane's latest launch
        hipEvent_t ev_prev;       // ... and behind the one before it (the two handles swap at every launch)
        bool used;                // ev has been recorded at least once
        bool used_prev;           // ev_prev too
        bool need_fork;           // the control stream has had work since this lane last looked: wait for ev_fork first
        const void* rd[3];        // operand ranges of the latest launch: inputs ...
        size_t rd_bytes[3];
        const void* wr[3];        // ... and outputs
        size_t wr_bytes[3];
    } lane[2];
    void* d_Lspill_lane1;         // lane 1's own copy of the per-bin scratch slots (orders 33..64), allocated when pipelining is switched on
    int n_lanes;                  // 1: every launch on `stream` (the default), 2: pipelined
    int lane_next;
    bool ctrl_dirty;              // work has been put on the control stream that the lanes have not been ordered behind yet
    hipEvent_t ev_fork;
    std::string err;
};

void apv_stream_free(apv_handle* h);      // stream.hip
void apv_bb_free(apv_handle* h);          // stream_bb.hip
long apv_bb_not_converged(const apv_handle* h);   // stream_bb.hip: hops of the broadband stream that hit the sweep cap
void apv_gevd_large_free(apv_handle* h);  // kernels_gevd_large.hip
void apv_gevd_lead_free(apv_handle* h);   // kernels_gevd_lead.hip
int apv_fail(apv_handle* h, int code, const std::string& msg);
// sink != nullptr: apv_fail on the calling thread writes its message to *sink instead of the handle, until called with nullptr.  A
// helper thread of a call sets it, so that h->err has one writer: the thread that returns the call's code.
void apv_fail_redirect(std::string* sink);
GevdParams apv_base_params(const apv_handle* h);
// the launch's first (or only) zone program is program `zone`: its row of the span's tables and outputs becomes span.z[0]
inline void apv_span_first_zone(GevdParams& p, int zone) { if (zone) p.span.z[0] = p.span.z[1]; }

// hipFuncSetAttribute(kernel, MaxDynamicSharedMemorySize, bytes) on the current device, once per device: the attribute is the
// device's.  `done` is the caller's static record for this kernel, bit d for device d (from device 64 on: set at every call).
inline hipError_t apv_set_max_dynamic_lds(const void* kernel, int bytes, std::atomic<unsigned long long>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = dev < 64 ? 1ull << dev : 0;
    if (done.load(std::memory_order_relaxed) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_relaxed);
    return e;
}

// kernels_gevd.hip.  Orders 65..128 go to kernels_gevd128.hip; ranks_all: the whole rank list when p.nV > APV_MAX_RANKS (only
// that kernel reads more than p.ranks), else nullptr
hipError_t apv_launch_gevd(const GevdParams& p, int compute_dtype, bool fused, hipStream_t s, std::string* why,
                           const int32_t* ranks_all = nullptr);
int apv_gevd_reads_groups(const GevdParams& p, int compute_dtype, bool x_c128);      // bins per group of the spectra layout that launch reads (1: bin-major)
// HBM scratch the kernel that WILL run needs for K bins of order n (0 for most configurations): the order-64 kernel's slots when
// it is eligible, the float64 LDS kernel's parked Cholesky factor at orders 33..64 otherwise.  zones: 1 or 2 zone programs.
size_t apv_gevd_spill_bytes(int n, int K, int compute_dtype, int reg_mode, double reg_bright, double sweep_tol2, int zones);
bool apv_gevd64_eligible(int n, int reg_mode, double reg_bright, double sweep_tol2);

// kernels_gevd128.hip: orders 65..128 in float64 arithmetic (packed LDS Cholesky, whitening, Householder tridiagonalisation,
// implicit QL).  Needs p.Lspill with apv_gevd_spill_bytes() bytes: per (zone program, bin) a slot of apv_gevd128_slot_bytes(n).
// A fused launch first writes R_B, R_D, r into the slots (corr128_kernel).
hipError_t apv_launch_gevd128(const GevdParams& p, int compute_dtype, bool fused, hipStream_t s, std::string* why,
                              const int32_t* ranks_all);
size_t apv_gevd128_slot_bytes(int n);
// R_B, R_D [K][L][L] and r [K][L] c128 from bin-major c64 (x_c128 = 0) or c128 slabs, L <= 128
hipError_t apv_launch_corr128(int K, int M, int L, int x_c128, const void* XB, const void* XD, const void* d, double2* RB,
                              double2* RD, double2* r, hipStream_t s);

// kernels_gevd16m.hip: order-16 fast path (MFMA correlation / whitening / back-transform + register-resident
// Jacobi); hipErrorNotSupported when the problem does not qualify
hipError_t apv_launch_gevd16m(const GevdParams& p, int compute_dtype, bool fused, hipStream_t s);
bool apv_gevd16m_takes_hops(const GevdParams& p, int compute_dtype, bool fused);      // would that launch accept p.n_hops > 1?

// kernels_gevd64.hip: order-64 float64 path (float32 block Jacobi on the f32 MFMA + float64 refinement on the f64 MFMA);
// hipErrorNotSupported when the problem does not qualify.  Needs p.Lspill with apv_gevd_spill_bytes() bytes.
hipError_t apv_launch_gevd64(const GevdParams& p, int compute_dtype, bool fused, hipStream_t s);
size_t apv_gevd64_slot_bytes();          // scratch per (zone program, bin)

// kernels_gevd_large.hip: real symmetric pairs of broadband order, f64, device pointers (see the file header)
int apv_gevd_large(apv_handle* h, int n, int batch, const double* d_A, const double* d_B, double reg,
                   const double* d_reg_scale, double* d_U, double* d_lam, const double* d_r, double mu, int V, const int* d_ranks, double* d_w, int32_t* h_status);

// kernels_gevd_lead.hip: the leading b eigenpairs of whitened matrices by Chebyshev-filtered subspace iteration (see the file header)
int apv_gevd_lead_block(int n, int rank);
// blocks of page-locked host memory handed out by apv_host_alloc (capi.hip)
void apv_host_blocks_note(const void* p, size_t bytes, bool add);
bool apv_host_block_contains(const void* p, size_t bytes);
int apv_gevd_lead(apv_handle* h, int n, int ne, int batch, int b, int rank, const double* C, const double* WT, double* d_U,
                  double* d_lam, const int* h_pd_flags, int* done);

// kernels_norm2.hip: d_out[i] = ||mats[i]||_2 (largest eigenvalue of a symmetric PSD n x n matrix, Lanczos), i < count <= 4,
// n <= APV_NORM2_MAX_N.  method: APV_NORM2_AUTO (the chip-wide steps above APV_NORM2_GRID_MIN_N, else one workgroup per
// matrix), APV_NORM2_ONE_WG or APV_NORM2_GRID (include/apvast_hip.h).
constexpr int APV_NORM2_MAX_N = 4096;
constexpr int APV_NORM2_GRID_MIN_N = 2048;      // the chip-wide path runs from n = 2049
hipError_t apv_launch_norm2(int n, int count, const double* const* d_mats, double* d_out, hipStream_t s, int method = APV_NORM2_AUTO);

// kernels_corr.hip
hipError_t apv_launch_corr(int compute_dtype, int K, int M, int L, const float2* XB, const float2* XD,
                           const float2* d, void* RB, void* RD, void* r, hipStream_t s);

hipError_t apv_launch_corr_c128(int K, int M, int L, const double2* XB, const double2* XD, const double2* d, double2* RB,
                                double2* RD, double2* r, hipStream_t s);

// bf16 inputs ((re, im) bf16 pairs, 4 B per element), f32 accumulation on v_mfma_f32_32x32x16_bf16; L in {32, 64}
hipError_t apv_launch_corr_bf16(int K, int M, int L, const uint32_t* XB, const uint32_t* XD, const uint32_t* d,
                                float2* RB, float2* RD, float2* r, hipStream_t s);
hipError_t apv_launch_to_bf16(size_t count, const float2* in, uint32_t* out, hipStream_t s);

// kernels_statwin.hip: statistics of the subband stream over a window of T hops (see the file header).  One launch per hop for
// `zones` zone programs: the hop's Gram matrices into slot ctr[0] of the rings, the window sums (oldest slot first) into RB / RD /
// r, then the counters ctr = {head, fill} advanced by a second, one-thread launch.
size_t apv_statwin_slot_elems(int L);         // complex elements of one bin's ring slot: 2 L^2 + L
hipError_t apv_launch_statwin(int x_c128, int acc_f64, int K, int M, int L, int T, int zones, const void* const* XB,
                              const void* const* XD, const void* const* d, void* const* ring, void* const* RB, void* const* RD,
                              void* const* r, int32_t* ctr, hipStream_t s);
// ... and with exponential forgetting: acc <- beta acc + (the hop's Gram matrices) in ONE slot per zone program, the new sums
// into RB / RD / r.  One launch, no counters.
hipError_t apv_launch_statforget(int x_c128, int acc_f64, int K, int M, int L, double beta, int zones, const void* const* XB,
                                 const void* const* XD, const void* const* d, void* const* acc, void* const* RB, void* const* RD,
                                 void* const* r, hipStream_t s);
hipError_t apv_launch_widen_c64(size_t count, const void* in, void* out, hipStream_t s);     // c64 -> c128

// kernels_stft.hip
constexpr int APV_STFT_MAX_JOBS = 8;            // channel sets of one analysis launch (STFT_MAX_JOBS there)
hipError_t apv_launch_stft_analysis(int N, int n_ch, const float* x, float2* spec, hipStream_t s, std::string* why);
hipError_t apv_launch_istft_ola(int N, int H, int n_ch, const float2* spec, float* overlap, float* out,
                                hipStream_t s, std::string* why);
hipError_t apv_launch_stft_analysis_jobs(int f64, int N, int n_jobs, const void* const* x, const int* n_ch, void* const* spec,
                                         const long* stride_c, const long* stride_k, int ring_off, hipStream_t s,
                                         std::string* why);
hipError_t apv_launch_stft_analysis_strided(int N, int n_ch, const float* x, int ring_off, float2* spec,
                                            long stride_c, long stride_k, hipStream_t s, std::string* why);
hipError_t apv_launch_istft_ola_strided(int N, int H, int n_ch, const float2* spec, long stride_c, long stride_k,
                                        float* overlap, float* out, hipStream_t s, std::string* why);

bool apv_stft_size_ok(int N, std::string* why);
hipError_t apv_stft_prepare(int N, int f64);
// general forms: f64 = 0/1 selects float/double data; in_len < N zero-pads; use_win = 0 skips the sine window
hipError_t apv_launch_analysis(int f64, int N, int n_ch, const void* x, long x_stride, int in_len, int ring_off,
                               int use_win, void* spec, long stride_c, long stride_k, hipStream_t s, std::string* why);
// out_group > 0 (and dividing n_ch): the emitted hop is written sample-major in groups of out_group channels, [n_ch / out_group][H]
// [out_group], instead of channel-major [n_ch][H]; out_gstride > 0: elements between two groups (default H out_group)
hipError_t apv_launch_synthesis(int f64, int N, int H, int n_ch, const void* spec, long stride_c, long stride_k,
                                void* overlap, void* out, hipStream_t s, std::string* why, int out_group = 0, long out_gstride = 0);
// K1 (RIR convolution of a hop) by fast convolution, float (f64 = 0) or double data: see fir_fft_kernel
int apv_fir_fft_size(int f64, int P, int H);       // segment length F, 0 = use the direct form
hipError_t apv_launch_fir_spectra(int f64, int F, int n_ch, const void* x, int P, void* Hf, hipStream_t s, std::string* why);
hipError_t apv_launch_fir_input_spectra(int f64, int F, const void* x0, const void* x1, int in_len, void* Xf, hipStream_t s);
hipError_t apv_launch_fir_chunk_spectra(int f64, int F, int P, int H, int n_hops, const void* hist0, const void* hist1,
                                        const void* pin, void* Xf, hipStream_t s);
// n_part > 1: uniformly partitioned (partitions of H taps, F = 2 H): Hf[j] is [n_part][C_j][F/2 + 1], Xf[j] points at the job's
// signal inside [n_part][2][F/2 + 1]
hipError_t apv_launch_fir_fft_jobs(int f64, int F, int n_jobs, const void* const* Hf, const void* const* Xf, void* const* resp,
                                   const int* n_ch, int P, int H, int N, int ring_off, hipStream_t s, int n_part = 1);
hipError_t apv_launch_fir_input_spectra_parts(int f64, int F, int n_part, const void* x0, const void* x1, void* Xf, hipStream_t s);
hipError_t apv_launch_fir_spectra_part(int f64, int F, int n_ch, const void* x, long x_stride, int taps, void* Hf, hipStream_t s,
                                       std::string* why);
// uniformly partitioned K1 for (P, H): number of partitions (segments of 2 H samples), 0 when it does not apply
int apv_fir_partitions(int f64, int P, int H);

// kernels_constrain.hip: the filter-length constraint.  w[z] [N/2 + 1][nV][L] complex (c128: double, else float) of `zones` zone
// programs projected in place onto the spectra of J-tap responses, the taps to taps[z] [nV][J][L] real of the same precision
// (taps, or an entry of it, may be null).  One launch; the tables of (N, precision) must exist when it is captured (apv_stft_prepare)
bool apv_constrain_size_ok(int c128, int N, std::string* why);
hipError_t apv_launch_constrain_filters(int c128, int N, int J, int nV, int L, int zones, void* const* w, void* const* taps,
                                        hipStream_t s, std::string* why);
// ... of the n_hops filter sets w[z] + i hop_w, taps to taps[z] + i hop_taps (strides in elements), in one launch (grid.z = hop x zone)
hipError_t apv_launch_constrain_filters_hops(int c128, int N, int J, int nV, int L, int zones, void* const* w, void* const* taps,
                                             int n_hops, size_t hop_w, size_t hop_taps, hipStream_t s, std::string* why);

// kernels_effort.hip: the array-effort limit (see the file header).  The filters w[z] [K][nV][L] complex (c128: double, else
// float) of `zones` zone programs and n_hops hops (hop i at w[z] + i hop_w elements) limited in place by limit[z] [K], one launch.
constexpr int APV_EFFORT_MAX_SLOTS = APV_MAX_SRCS;     // nV of a launch
constexpr int EFFORT_EMIT_NONE = -1, EFFORT_EMIT_ALL = -2;
struct EffortArgs {
    void* w[2];
    const double* limit[2];
    double* effort[2];             // outputs (may be null with EFFORT_EMIT_NONE): [K][nV], ...
    int32_t* src[2];               // ... [K] ...
    double* gain[2];               // ... [K]
    int zones = 1, n_hops = 1;
    size_t hop_w = 0;
    int emit_hop = 0;              // the hop that writes the outputs; EFFORT_EMIT_ALL: every hop, hop i's hop_bins bins further on
    size_t hop_bins = 0;
};
hipError_t apv_launch_limit_effort(int c128, int K, int nV, int L, const EffortArgs& a, hipStream_t s, std::string* why);

// kernels_valspan.hip: the rank choice by the contrast at validation microphones (see the file header).  The filters w[z]
// [K][nV][L] complex (c128: double, else float) of `zones` zone programs, replaced in place from the energies their slots put on
// the banks g_bright[z] / g_dark[z] [K][Mv][L] complex128 under the floor phi[z] [K], one launch.
constexpr int APV_VALSPAN_MAX_SLOTS = APV_MAX_SRCS;    // nV of a launch
struct ValSpanArgs {
    void* w[2];
    const void* g_bright[2];       // the bank of the program's own zone ...
    const void* g_dark[2];         // ... and of the other zone
    const double* phi[2];
    double* bright[2];             // outputs (may be null with emit = 0): [K][nV], ...
    double* dark[2];               // ... [K][nV] ...
    int32_t* src[2];               // ... [K][nV]
    int zones = 1;
    int emit = 1;                  // 0: the launch writes the filters alone
};
hipError_t apv_launch_validation_span(int c128, int K, int nV, int L, int Mv, const ValSpanArgs& a, hipStream_t s, std::string* why);

// kernels_firsynth.hip: the FIR synthesis of a constrained stream (see the file header).  One launch writes the groups
// [program 0: nV][program 1: nV][target A][target B] (n_tgt = 0: no target groups) of H samples x L loudspeakers each; element
// (g, n, l) of the result goes to out[g H L + n sn + l sl].  Taps are float or double (taps_f64), samples and results likewise (x_f64).
struct FirSynthArgs {
    const void* prev[2];           // per zone program of the launch: the taps the hop fades from, [nV][J][L]
    const void* cur[2];            // ... and the hop's own
    int sig[2];                    // the input signal each program filters
    const void* xhist[2];          // per input signal: the J - 1 samples in front of the hop, oldest first (not read when J = 1)
    const void* xhop[2];           // ... and the hop's H samples
    int nz, nV, L, J, H;
    int n_tgt, ref, delay;         // target groups: x[n - delay] in column ref, zeros elsewhere
    void* out;
    long sn, sl;
    // a chunk of hops in ONE launch (chunked whole-signal path; blockIdx.z = hop x group): n_hops <= 1 is a single hop and the three
    // strides are not used.  Hop i takes its taps from cur[z] + i hop_taps (elements) and fades from the taps of hop i - 1 there
    // (hop 0: from prev[z]); its samples are xhist[g] + i hop_x and xhop[g] + i hop_x (elements: hop_x = H and xhop = xhist + J - 1
    // read one linear row [J - 1 samples before the chunk | the chunk]); its result starts hop_out BYTES behind that of hop i - 1
    int n_hops;
    size_t hop_taps, hop_x, hop_out;
};
hipError_t apv_launch_fir_synthesis(int taps_f64, int x_f64, const FirSynthArgs& a, hipStream_t s, std::string* why);
// behind it: prev[z] <- cur[z] (n_taps elements each), new_hist[g] <- the J - 1 newest samples of [old_hist[g] | xhop[g]], g < 2
struct FirSynthAdvance {
    const void* cur[2];
    void* prev[2];
    size_t n_taps;
    const void* old_hist[2];
    const void* xhop[2];
    void* new_hist[2];
    int nz, J, H;
};
hipError_t apv_launch_fir_synth_advance(int taps_f64, int x_f64, const FirSynthAdvance& a, hipStream_t s);
// the linear input rows of a chunk of nc hops, rows[g] = [J - 1 samples before the chunk | nc H samples of the chunk] for the two
// input signals: the head from head[g] + head_off (the synthesis' history, or the tail of the previous chunk's rows), the body from
// the pinned staging pin [nc][2][H]; samples float or double (x_f64).  head and rows must not overlap
hipError_t apv_launch_fir_synth_rows(int x_f64, int J, int H, int nc, const void* const head[2], size_t head_off, const void* pin,
                                     void* const rows[2], hipStream_t s);

// kernels_streameval.hip: the evaluation stage of the subband stream (see the file header).  One launch computes the pressures
// p [n_sets][H][Mv] (float64) of n_sets pressure sets; set i filters group map[4 i] of the hop's result buffer -- element (g, n, l)
// at hop[g hop_stride + n sn + l sl], with the Pv - 1 samples in front of the hop at hist[map[4 i + 1] hist_stride + q L + l] --
// through the bank rv[map[4 i + 2]] [Pv][L][Mv].  map = nullptr: set i reads group i, history i, bank 0.  Samples float or double
// (x_f64); banks and pressures float64.
struct EvalPressureArgs {
    const void* hist;
    const void* hop;
    size_t hist_stride, hop_stride;
    long sn, sl;
    const double* rv[2];
    const int32_t* map;
    double* p;
    int n_sets, Pv, H, L, Mv;
};
bool apv_eval_pressure_fits(int Pv);           // one loudspeaker's window fits LDS: Pv <= 20465
// outside a capture, once per (precision, geometry): lets the kernel that (Pv, H, L) selects use more than 64 KB of LDS where it must
hipError_t apv_eval_pressure_prepare(int x_f64, int Pv, int H, int L);
hipError_t apv_launch_eval_pressure(int x_f64, const EvalPressureArgs& a, hipStream_t s, std::string* why);
// behind it: the energies of the hop from p [Z][2 E + 1][H][Mv] (per program: bright of E ranks, dark of E ranks, target) into slot
// ctl[2 + par] of the record at ctl[0] (ctl[1] slots; [Z][3 E + 1][Mv] per slot: bright, dark, error per rank, target) and added to
// totals; ctl[2 + (par ^ 1)] <- slot + 1; new_hist[g] <- the Pv - 1 newest samples of [old_hist[g] | group hist_src[g] of the hop]
struct EvalAdvanceArgs {
    const double* p;
    double* totals;
    unsigned long long* ctl;
    int par;
    const void* old_hist;
    void* new_hist;
    const void* hop;
    size_t hop_stride;
    long sn, sl;
    const int32_t* hist_src;
    int Z, E, H, Mv, Pv, L, n_hist;
};
hipError_t apv_launch_eval_advance(int x_f64, const EvalAdvanceArgs& a, hipStream_t s);

// kernels_bbeval.hip: the evaluation stage of the broadband stream behind a pressure launch over n hops (see the file header).
// p [Z][2 E + 1][n H][Mv] -> the energies of hop i into slot slot0 + i of rec (slots of [Z][3 E + 1][Mv]); the order of a hop's sum
// depends on H alone.
struct BbEvalEnergyArgs {
    const double* p;
    double* rec;
    int slot0, Z, E, H, Mv, n;
};
bool apv_bbeval_sizes_ok(int Z, int E, int H, int Mv, int n, std::string* why);
hipError_t apv_launch_bbeval_energies(const BbEvalEnergyArgs& a, hipStream_t s, std::string* why);
// behind it: totals <- totals + slot, for the slots slot0 .. slot0 + n - 1 in order; and with Pv > 1 and n_hist > 0, new_hist[g]
// [Pv - 1][L] <- the newest Pv - 1 samples of [old_hist[g] | the n H samples of group hist_src[g]], sample (g, t, l) of the launch at
// hop[g hop_stride + t sn + l sl].  Everything float64.
struct BbEvalAdvanceArgs {
    const double* rec;
    double* totals;
    const double* old_hist;
    double* new_hist;
    const double* hop;
    size_t hop_stride;
    long sn, sl;
    const int32_t* hist_src;
    int slot0, Z, E, H, Mv, n, Pv, L, n_hist;
};
hipError_t apv_launch_bbeval_advance(const BbEvalAdvanceArgs& a, hipStream_t s);

// kernels_evalspec.hip: per-bin evaluation spectra (see the file header).  Three launches behind the two above: the hop's
// pressures p [Z (2 E + 1)][H][Mv] into the ring [Z (2 E + 1) Mv][N] at the stream's ring offset (the offset AFTER the hop's
// advance, as K1 and the analysis take it), the windowed float64 transform of every ring row into spec [N/2 + 1][Z (2 E + 1) Mv]
// complex128, and |P|^2 added to totals [Z][3 E + 1][N/2 + 1][Mv].  The float64 tables of N must exist when it is captured
// (apv_stft_prepare(N, 1)).
struct EvalSpectraArgs {
    const double* p;
    double* ring;
    void* spec;
    double* totals;
    int ring_off, N, H, Z, E, Mv;
};
bool apv_eval_spectra_size_ok(int N, int H, int Z, int E, int Mv, std::string* why);
hipError_t apv_launch_eval_spectra(const EvalSpectraArgs& a, hipStream_t s, std::string* why);

// kernels_bbevalspec.hip: the same spectra for the broadband stream, n consecutive hops per call (see the file header).  p: the
// pressures [Z (2 E + 1)][.. n H ..][Mv] of the n hops, the sets p_set elements apart.  line[cur] holds the current line
// [Z (2 E + 1) Mv][len], len >= N - H, whose last N - H samples are the newest from before the call; the call runs the n hops as
// sub-launches of at most per_launch hops -- line [Z (2 E + 1) Mv][N - H + c H] into the other buffer, the windowed float64
// transforms of its c frames into spec [c][N/2 + 1][Z (2 E + 1) Mv] complex128, |P|^2 added to totals [Z][3 E + 1][N/2 + 1][Mv]
// in hop order -- and leaves cur and len at the last line.  Both line buffers hold N - H + min(n, per_launch) H samples per
// channel, spec min(n, per_launch) hops.  The float64 tables of N must exist (apv_stft_prepare(N, 1)).
constexpr size_t APV_BBSPEC_SCRATCH_BYTES = (size_t)64 << 20;       // budget of spec; one hop where a hop is larger
// the optional detectability part (kernels_evaldetect.hip, hop-batched): behind every sub-launch's transforms, on its scratch,
// before the next sub-launch overwrites it.  curves and part hold min(n, per_launch) hops; hop i of the call goes to slot
// slot0 + i of rec.
struct BbSpecDetectArgs {
    const double* G2T;
    const double* quiet;
    double* curves;
    double* part;
    double* rec;
    double* totals;
    int slot0, C;
    double Cs, Ca, Leff;
};
struct BbSpecArgs {
    const double* p;
    size_t p_set;
    double* line[2];
    int cur;
    long long len;
    void* spec;
    double* totals;
    int N, H, Z, E, Mv, n, per_launch;
    const BbSpecDetectArgs* detect;  // null: off
};
bool apv_bbspec_size_ok(int N, int H, int Z, int E, int Mv, std::string* why);
int apv_bbspec_hops_fit(int N, int Z, int E, int Mv);         // hops per sub-launch the budget allows, at least 1
hipError_t apv_launch_bbspec_hops(BbSpecArgs* a, hipStream_t s, std::string* why);
// the detectability part alone on a caller's spectra [n][N/2 + 1][Z (2 E + 1) Mv], in sub-launches of at most per_launch hops as
// above (d.slot0 the slot of the first hop; d.curves and d.part hold min(n, per_launch) hops)
hipError_t apv_launch_bbspec_detect_hops(const BbSpecDetectArgs& d, const void* spec, int n, int per_launch, int N, int Z, int E, int Mv,
                                         hipStream_t s, std::string* why);

// kernels_evaldetect.hip: perceptual detectability of the evaluated pressures (see the file header).  Three launches behind the
// spectra above, on their bin-major scratch spec [N/2 + 1][Z (2 E + 1) Mv]: the squared weighting curves of the Z Mv target
// spectra into curves [N/2 + 1][Z Mv], the weighted sums of every (program, rank, microphone) over the bins 1.. as `chunks`
// partial sums into part [chunks][Z][2 E][Mv] (per program: error of the E ranks, leak of the E ranks), and their sum, in chunk
// order, into the hop's slot [Z][2 E][Mv] and the totals [Z][6 E][Mv] (per program: sum, max, count of D > 1 of the error, then of
// the leak).  The slot is `hop`, or where that is null slot ctl[2] - 1 of the record at ctl[0] (ctl[1] slots), ctl[2] the hops of the
// call so far, which the first launch advances.  G2T [C][N/2 + 1]: the model's squared channel responses, channel-major; quiet
// [N/2 + 1]: the curve of a silent masker (apv_launch_eval_detect_quiet), read where Z = 1.
struct EvalDetectArgs {
    const void* spec;
    const double* G2T;
    const double* quiet;
    double* curves;
    double* part;
    double* hop;
    unsigned long long* ctl;
    double* totals;
    int N, Z, E, Mv, C;
    double Cs, Ca, Leff;
};
bool apv_eval_detect_size_ok(int N, int Z, int E, int Mv, int C, std::string* why);
int apv_eval_detect_chunks(int N, int Z, int E, int Mv);      // partial sums per element: a function of the sizes alone
hipError_t apv_launch_eval_detect_quiet(int N, int C, const double* G2T, double Cs, double Ca, double Leff, double* quiet, hipStream_t s);
hipError_t apv_launch_eval_detect(const EvalDetectArgs& a, hipStream_t s, std::string* why);
// the hop-batched form, on the spectra of n consecutive hops spec [n][N/2 + 1][Z (2 E + 1) Mv]: curves [n][N/2 + 1][Z Mv], part
// [n][chunks][Z][2 E][Mv], hop i into slot slot0 + i of rec (slots of [Z][2 E][Mv]) and, in hop order, into the totals.  n <= 65535.
struct EvalDetectHopsArgs {
    const void* spec;
    const double* G2T;
    const double* quiet;
    double* curves;
    double* part;
    double* rec;
    double* totals;
    int slot0, n, N, Z, E, Mv, C;
    double Cs, Ca, Leff;
};
hipError_t apv_launch_eval_detect_hops(const EvalDetectHopsArgs& a, hipStream_t s, std::string* why);

// whole-signal path, a chunk of hops per launch (kernels_stft.hip / kernels_stream.hip; see process_signal_chunked_t in stream.hip)
hipError_t apv_launch_stft_analysis_chunk(int f64, int N, int n_jobs, const void* const* x, const int* n_ch, void* const* spec,
                                          const long* stride_c, const long* stride_k, long x_stride, long x_hop, const long* spec_hop,
                                          int n_hops, hipStream_t s, std::string* why);
hipError_t apv_launch_fir_fft_chunk(int f64, int F, int n_jobs, const void* const* Hf, const void* const* Xf, long x_hop_stride,
                                    void* const* resp, const int* n_ch, int P, int H, int row_stride, int pos0, int n_hops,
                                    hipStream_t s);
hipError_t apv_launch_rows_copy(int f64, int rows, int len, void* dst, long ds, int d0, int dmod, const void* src, long ss, int s0,
                                int smod, hipStream_t s);
hipError_t apv_launch_chunk_inputs(int f64, int P, int H, int N, int nc, int pad, int RL, const void* const old_hist[2],
                                   void* const new_hist[2], const void* pin, void* inL, hipStream_t s);

// kernels_stream.hip
struct FirJob { const float* rir; const float* xh; float* resp; int C; };
struct FirJobs { FirJob j[6]; int n; };
// all FIR jobs of a hop in one launch, on the matrix cores (v_mfma_f32_32x32x2_f32, implicit Toeplitz operand)
hipError_t apv_launch_fir_jobs(const FirJobs& jobs, int P, int H, int N, int ring_off, hipStream_t s);
// float64 jobs of one hop on v_mfma_f64_16x16x4_f64 (both stream modes); tile0 is filled by the launcher
constexpr int FIR_JOBS_D = 6;
struct FirJobsD {
    const double* rir[FIR_JOBS_D];     // [P][C_j]
    const double* xh[FIR_JOBS_D];      // input history of the job's signal
    double* resp[FIR_JOBS_D];          // [C_j][N] ring
    int C[FIR_JOBS_D];
    int tile0[FIR_JOBS_D + 1];         // first channel tile of each job
};
hipError_t apv_launch_fir_jobs_f64(FirJobsD jobs, int njobs, int P, int H, int N, int ring_off, hipStream_t s);
int apv_fir_pad_f64();
// kernels_bb.hip: the broadband stream's own stages, float64 (the comments of the kernels say what each computes)
struct SyrkJobs {
    const double* stats[4];
    double* R[4];
};
// up to four channel groups with inputs of their own, one launch (a hop's zone programs and target paths)
struct ApplyJobsD {
    const double2* in[4];
    const double2* filt[4];
    double2* out[4];
    int first[5];          // first channel of each job in the launch's channel index; first[n] = total
    int n;
};
// both input signals' histories: new = [old[H:], x, zeros(pad)], x [2][H]
hipError_t apv_launch_hist2_f64(int P, int H, int pad, const double* old0, const double* old1, const double* x, double* new0,
                                double* new1, hipStream_t s);
// ring[c][(len - H + n + off) % len] = src[c][n], n < H, c < n_ch
hipError_t apv_launch_ring_append_f64(int len, int H, int off, const double* src, long src_ld, double* ring, int n_ch, hipStream_t s);
// R = sum_m Y_m Y_m^T of njobs Hankel data matrices (displacement form where it fits, else dense products on the matrix cores).
// form: APV_HANKEL_AUTO is that choice; APV_HANKEL_DISPLACEMENT / APV_HANKEL_DENSE force one (the displacement form where it
// does not fit: hipErrorInvalidValue, nothing launched).  *form_taken: the form that was launched.
hipError_t apv_launch_syrk_hankel(hipStream_t s, int n, int J, int L, int M, int S, int off, int skip, int ncols, int njobs,
                                  const SyrkJobs& jobs, int form = APV_HANKEL_AUTO, int* form_taken = nullptr);
// r = sum_m Y_m d_m[toff:]
hipError_t apv_launch_xcorr_hankel(int n, int J, int L, int M, int S, int off, int skip, int ncols, int toff, const double* stats,
                                   const double* tstats, double* r, hipStream_t s);
// R[i][i] += coef * nrm[0]
hipError_t apv_launch_add_rel_diag(int n, double* R, double coef, const double* nrm, hipStream_t s);
// out[q][ch][k] = in[q][k] * filt[q][ch][k] over the jobs' j.first[j.n] channels
hipError_t apv_launch_apply_jobs_f64(int K, const ApplyJobsD& j, hipStream_t s);
// p[t][m] = sum_s sum_q rir[q][s][m] x[t-q][s], M <= 256
hipError_t apv_launch_predict_pressure(int T, int L, int M, int P, const double* x, const double* rir, double* out, hipStream_t s);
// v[i] *= f
hipError_t apv_launch_scale_f64(size_t count, double* v, double f, hipStream_t s);
// kernels_live.hip: responses reassigned between hops (apv_stream_set_rirs / apv_bb_set_rirs).  Jobs 0..3 are the paths A->A, A->B,
// B->A, B->B ([C][P-1] tails), 4..5 the targets ([M][P-1]); all buffers in the stream's front-end precision.
struct FirLive {
    int hops_left;                 // hops whose K1 output still takes a tail (0: nothing pending, the stream runs as if never updated)
    bool live[6];                  // job j has a tail
    void* corr[6];                 // tails [C_j][P-1], index 0 = the next hop's first sample; allocated at the first update
    void* stage[4];                // new banks rir A, B, trir A, B in the device layout, on their way in
};
struct FirLiveJobs {
    const void* old[FIR_JOBS_D];   // fir_tail: bank as it was, bank that replaces it, the P - 1 newest input samples
    const void* nw[FIR_JOBS_D];
    const void* xh[FIR_JOBS_D];
    void* corr[FIR_JOBS_D];
    void* dst[FIR_JOBS_D];         // tail_apply: K1 output rows
    int C[FIR_JOBS_D];
    int n;
};
struct FirLiveBanks {
    int P, H, L, M, f64;
    void* rir[2];                  // [P][C] banks of the stream, rewritten in place
    void* trir[2];                 // [P][M]
    const void* hist_tail[2];      // per signal: the P - 1 newest input samples before the update, oldest first
};
hipError_t apv_launch_fir_tail(int f64, const FirLiveJobs& jobs, int P, hipStream_t s);
hipError_t apv_launch_tail_apply(int f64, const FirLiveJobs& jobs, int Q, int n_add, int shift, long row_len, int d0, int dmod,
                                 hipStream_t s);
hipError_t apv_launch_bank_transpose(int f64, int P, int C, const void* src, void* dst, hipStream_t s);
void apv_bank_to_device(const double* src, int P, int L, int M, bool target, std::vector<double>& out);
// the changed banks (h_new[k] != nullptr: rir A, rir B, target A, target B) uploaded, their tails accumulated, the banks replaced
int apv_live_update(apv_handle* h, FirLive& fl, const FirLiveBanks& b, const double* const h_new[4], hipStream_t st);
// after K1: the next n_add samples of every live tail added to dst[j] at (d0 + m) mod dmod (rows row_len apart), tails shifted by `shift`
int apv_live_apply(apv_handle* h, FirLive& fl, int P, int C, int M, int f64, void* const dst[6], int n_add, int shift, long row_len,
                   int d0, int dmod, hipStream_t st);
void apv_live_advance(FirLive& fl, int hops);
// state names of an indexed family, "<pre><c>" with c one of the `count` characters from `first` on ('0': an index, 'A': a zone
// program): c - first, else -1
inline int apv_name_index(const char* name, const char* pre, int count, char first = '0') {
    const size_t pl = std::strlen(pre);
    if (std::strncmp(name, pre, pl) != 0 || name[pl] == 0 || name[pl + 1] != 0) return -1;
    const int q = name[pl] - first;
    return q >= 0 && q < count ? q : -1;
}
// named state "fir_correction<j>" (j < 4) / "target_fir_correction<j - 4>" of either stream: j, else -1 ...
inline int apv_live_index(const char* name) {
    const int p = apv_name_index(name, "fir_correction", 4), z = apv_name_index(name, "target_fir_correction", 2);
    return p >= 0 ? p : z >= 0 ? 4 + z : -1;
}
// ... and get or set tail j, esz bytes per sample
int apv_live_state(apv_handle* h, FirLive& fl, int j, int P, int H, int C, int M, size_t esz, void* h_buf, size_t bytes, bool get,
                   hipStream_t st);
void apv_live_free(FirLive& fl);
// f64 = 0: c64 spectra / float weights; 1: c128 spectra / double weights (bin-major [K][M])
hipError_t apv_launch_perceptual_weights(int f64, int K, int M, int nch, const void* spec, const double* G2, const double* G2T,
                                         double Cs, double Ca, double Leff, int N, int norm_mode, void* W, hipStream_t s);
hipError_t apv_launch_scale_spectra(int f64, int K, int C, int L, void* spec, const void* W, hipStream_t s);
hipError_t apv_launch_ungroup_spectra(int f64, int K, int C, int g, const void* in, void* out, hipStream_t s);
hipError_t apv_launch_perceptual_weights_f64(int K, int M, int nch, const double2* spec, const double* G2,
                                             const double* G2T, double Cs, double Ca, double Leff, int N, int norm_mode,
                                             double* W, hipStream_t s);
hipError_t apv_launch_scale_spectra_cm_f64(int K, int C, int L, double2* spec, const double* W, hipStream_t s);
hipError_t apv_launch_input_update(int f64, int P, int H, int pad, int N, int ring_off, const void* const old_hist[2],
                                   void* const new_hist[2], const void* xin, void* inblk, hipStream_t s);
int apv_fir_pad();
// out[ch][k] = in_spec[k] * filt(ch, k): ch < n_filt channels taken from the bin-major filter bank
// w[k][n_filt] (c64 or c128), remaining channels from the channel-major table tgt[ch - n_filt][k]
hipError_t apv_launch_apply_jobs(int K, int n_jobs, const void* const* in_spec, const void* const* w, const void* const* tgt,
                                 void* const* out, const int* n_filt, const int* n_tgt, int w_c128, int spec_f64, hipStream_t s);
