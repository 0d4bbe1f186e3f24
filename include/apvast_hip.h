/*
 * apvast_hip.h -- C ABI of the MI355X-native AP-VAST filter engine.
 *
 * This is the drop-in boundary for the per-block, per-subband hot path of the
 * reference (macoustics/ap-vast-unofficial).  The reference has no native code
 * and therefore no FFI of its own; each entry point below replaces a span of
 * NumPy/SciPy calls in Python/apvast.py, cited as "replaces:".  The host side
 * that binds it is ap_vast_unofficial_amd/_capi.py (ctypes); INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every function returns an int status: 0 = OK,
 *     negative = error (apv_last_error() gives the text).
 *   - complex numbers are interleaved (re, im) pairs: `float[2]` for c64,
 *     `double[2]` for c128.
 *   - a handle owns one HIP device, one stream, its workspaces and (optionally)
 *     one RCCL communicator.  Handles are thread-compatible, not thread-safe.
 *   - pointer arguments named h_* are HOST pointers, d_* are DEVICE pointers
 *     obtained from apv_dev_alloc() (or any hipMalloc'd memory on the handle's
 *     device).  No entry point allocates on the per-block path: apv_update_dev, apv_process_block*, apv_process_signal*
 *     and apv_bb_process_block use buffers sized by apv_create / apv_*_init (apv_process_signal sets up its second
 *     spectra set and pinned staging at its first call); the on-demand readers (apv_stream_get_statistics) allocate their
 *     work space once and keep it; the host-buffer conveniences (apv_update, apv_jdiag_*, apv_predict_pressure,
 *     apv_vast_static, apv_hankel_statistics) stage through device memory of their own.
 *
 * Data layout (HBM), subband mode -- bin-major so that one bin's control-point
 * matrix is one contiguous, coalesced slab:
 *   X_B, X_D : [K][M][L] c64   bright / dark control-point spectra of the K bins
 *                              owned by this handle; X[k] = spectra[k].T of
 *                              apvast.py:239-262, rows = control points (mics),
 *                              columns = loudspeakers (fastest).
 *   d        : [K][M]    c64   target spectrum at the bright control points
 *                              (apvast.py:199-209).
 *   w        : [K][nV][L] c64 (or c128)  VAST filter per bin and per rank V.
 *   lam      : [K][L]    f32 (or f64)    generalized eigenvalues, descending.
 *   status   : [K]       i32   0 OK; 1 = loaded R_D not positive definite
 *                              (numpy.linalg.LinAlgError at apvast.py:24);
 *                              2 = eigen-iteration did not converge.
 */
#ifndef APVAST_HIP_H
#define APVAST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APV_ABI_VERSION 2
#define APV_MAX_RANKS 64     /* number of simultaneously produced ranks V (nV) */
#define APV_MAX_N 64         /* largest GEVD order n = L of apv_jdiag_batched and of the per-bin kernels that hold the pair on-chip */
#define APV_MAX_SRCS 128     /* largest n_srcs of a handle: subband orders 65..128 take the packed float64 kernel (kernels_gevd128.hip) */
#define APV_MAX_STAT_HOPS 64 /* longest statistics window of the subband stream, in hops (apv_stream_set_stat_hops) */

/* status codes */
#define APV_OK 0
#define APV_ERR_ARG (-1)        /* invalid argument / unsupported size */
#define APV_ERR_HIP (-2)        /* HIP runtime error */
#define APV_ERR_NOT_PD (-3)     /* at least one bin: R_D + reg not positive definite */
#define APV_ERR_NO_CONVERGE (-4)/* at least one bin: eigen-iteration hit the sweep cap */
#define APV_ERR_RCCL (-5)       /* RCCL error / communicator not initialised */
#define APV_ERR_STATE (-6)      /* unknown state name / wrong size */

/* arithmetic the GEVD + filter run in (inputs are always c64) */
#define APV_F32 0
#define APV_F64 1

/* dark-matrix loading, apvast.py:22-27 */
#define APV_REG_ABS 0           /* B + reg_dark * I              (EXPERIMENTAL_REGULARIZATION=True) */
#define APV_REG_REL 1           /* B + reg_dark * ||B||_2 * I    (else-branch; MATLAB diagonalLoading) */

typedef struct apv_handle apv_handle;

#define APV_DIALECT_PYTHON 0   /* apvast.py: skipped sample in the data matrix, no normalisation, absolute dark loading, ranks 1..V */
#define APV_DIALECT_MATLAB 1   /* apVast.m: contiguous Hankel matrix, R and r / ((S-J+1) M), loading relative to ||R||_2, rank list */

typedef struct apv_config {
    int32_t abi_version;      /* APV_ABI_VERSION */
    int32_t device;           /* HIP device ordinal */
    int32_t n_bins;           /* K  : bins owned by this handle (its shard) */
    int32_t n_srcs;           /* L  : loudspeakers = GEVD order n (<= APV_MAX_SRCS; above APV_MAX_N the GEVD runs in float64 whatever
                                 compute_dtype is, outputs in the format out_c128 asks for) */
    int32_t n_mics;           /* M  : control points per zone */
    int32_t n_ranks;          /* nV : how many ranks V are produced (<= APV_MAX_RANKS; the reference emits every rank 1..V, apvast.py:406-422) */
    int32_t ranks[APV_MAX_RANKS]; /* the V list, each 1..L, ascending (longer lists: apv_set_rank_list) */
    int32_t compute_dtype;    /* APV_F32 | APV_F64 */
    int32_t out_c128;         /* 0: w c64 / lam f32;  1: w c128 / lam f64 */
    int32_t reg_mode;         /* APV_REG_ABS | APV_REG_REL */
    double  reg_dark;         /* 1e-7 in the Python dialect (apvast.py:23) */
    double  reg_bright;       /* relative bright loading (apVast.m:552-569); 0 in the Python dialect */
    double  mu;               /* trade-off parameter (apvast.py:49, 410) */
    int32_t max_sweeps;       /* Jacobi sweep cap; 0 = default.  Broadband mode: a value > 0 also selects the complete block-Jacobi solve for every hop (0: the per-hop path computes the leading eigenpairs the filters use, the rest when lambda / U are read) */
    int32_t block_size;       /* N : STFT length for the streaming entry points (0 = kernel-level use only); any even N in [4, 4096], above that up to 8192 with N/2 = 2^a 3^b 5^c 7^d (float32 front end) */
    int32_t hop_size;         /* H */
    int32_t n_zones;          /* streaming: bit mask of zone programs, 1 = A, 2 = B (run_A/run_B, apvast.py:53-54) */
    int32_t debug_stop;       /* profiling aid (0 = run everything): 1, 2, 3 stop the update kernels after stage n; the order-16 kernel also takes 4 (double sweeps only), 5 (guarded path always), 9 (mark bins by the refinement step they miss), 10 (guard off, results invalid); the order-64 kernel gives 4..8 its own meanings */
    int32_t dialect;          /* APV_DIALECT_PYTHON | APV_DIALECT_MATLAB: the broadband stream's statistics/loading/rank conventions */
    int32_t frontend;         /* streaming (subband) front-end precision -- RIRs, FIR, rings, STFT, spectra, overlap-add:
                                 0 = follow compute_dtype (APV_F64: everything float64, as the reference's lfilter / rfft /
                                 irfft are, apvast.py:171-192, 202-203, 461-496), 1 = float32, 2 = float64 */
    int32_t out_layout;       /* streaming (subband) outputs: 0 = channel-major h_out [n_out][H]; 1 = sample-major in groups of L channels
                                 (one zone program and rank each), h_out [n_out / L][H][L] -- the (hop, loudspeaker) arrays the
                                 reference's caller receives (apvast.py:498-504), so the host binding reshapes instead of
                                 transposing; apv_process_signal* then writes [n_out / L][n_hops * H][L] */
    int32_t reserved[4];
    double  sweep_tol2;       /* Jacobi stop threshold: a sweep whose pivots satisfy sum |c_pq|^2 <= sweep_tol2 ||C||_F^2 is the
                                 last one (quadratic convergence leaves ~sweep_tol2^2 behind).  0 = default (1e-16 in float64:
                                 csrc/gevd16_common.h Prec<double>, csrc/kernels_gevd.hip Tol<double>; 1e-8 in float32);
                                 apv_jdiag_* always iterate to 1e-17 */
} apv_config;

/* ---- lifetime ---------------------------------------------------------- */
int  apv_create(const apv_config* cfg, apv_handle** out);     /* replaces: apvast.__init__ allocation, apvast.py:115-151 */
int  apv_destroy(apv_handle* h);
const char* apv_last_error(const apv_handle* h);               /* h may be NULL: last create() error */
int  apv_abi_version(void);

/* Replace the subband rank list of cfg (n_ranks / ranks) by n ascending ranks in 1..n_srcs, 1 <= n <= n_srcs: the way to ask
 * for more than APV_MAX_RANKS ranks (the reference emits every rank 1..V, V <= L, apvast.py:152-154).  Output sizes follow
 * the new count (w is [K][n][L]).  Refused once apv_stream_init has run: the stream's buffers are sized there.
 *                                                         replaces apvast.py:152-154 */
int  apv_set_rank_list(apv_handle* h, int32_t n, const int32_t* ranks);

/* Statistics window of the subband stream: every bin's R_B, R_D, r are accumulated over the last n_hops hops,
 *   R_B[k] = sum_{t < n_hops} X_B^(h-t)[k]^H X_B^(h-t)[k]  (R_D likewise),  r[k] = sum_{t < n_hops} X_B^(h-t)[k]^H d^(h-t)[k],
 * the per-bin form of the reference's statistics buffer, which spans several blocks (512 samples against a block of 256 with
 * its example parameters); hops before the first contribute nothing.  n_hops in 1..APV_MAX_STAT_HOPS; 1 (the default) is the
 * single-block update that never writes R to HBM.  Above 1 every hop's Gram matrices go to a ring of n_hops slots sized by
 * apv_stream_init (n_hops x zone programs x K x (2 L^2 + L) complex of the compute precision; APV_ERR_HIP with the size in the
 * message if that cannot be allocated), the window sum feeds the explicit joint diagonalisation of apv_gevd_vast_dev,
 * apv_stream_get_statistics returns the windowed statistics, and the states "stat_window<z>" [n_hops][K][2 L^2 + L] (slots oldest
 * first, zero beyond the fill level) and "stat_window_fill" (one int32) carry the window for a resume.  Called between apv_create
 * and apv_stream_init; refused (APV_ERR_ARG, nothing changed) once the stream is initialised: the ring is sized there.
 *                                                         replaces: update_statistics' buffer of several blocks, apvast.py:329-364 */
int  apv_stream_set_stat_hops(apv_handle* h, int32_t n_hops);

/* Exponentially forgetting statistics of the subband stream: after hop h every bin holds
 *   R_B^(h)[k] = beta R_B^(h-1)[k] + X_B^(h)[k]^H X_B^(h)[k]  (R_D likewise),  r^(h)[k] = beta r^(h-1)[k] + X_B^(h)[k]^H d^(h)[k],
 * from R = 0, r = 0 before the first hop: the recursive form of the reference's statistics buffer, with one smoothing constant
 * in place of a window length and no ring.  beta in (0, 1]; 1 accumulates everything since the first hop.  apv_stream_init
 * allocates ONE slot per zone program (K x (2 L^2 + L) complex of the compute precision, zero-filled); every hop reads and
 * writes it once (one fma per real and imaginary part) and feeds the explicit joint diagonalisation of apv_gevd_vast_dev,
 * apv_stream_get_statistics returns the running sums, and the state "stat_forget<z>" [K][2 L^2 + L] carries them for a resume.
 * beta is fixed for the life of the stream.  Called between apv_create and apv_stream_init; refused (APV_ERR_ARG, nothing
 * changed) if beta is not a finite number in (0, 1], once the stream is initialised, or when a window of more than one hop is
 * set -- as apv_stream_set_stat_hops(h, n > 1) is once forgetting is set: the two exclude each other.
 *                                                         replaces: update_statistics' buffer of several blocks, apvast.py:329-364 */
int  apv_stream_set_stat_forgetting(apv_handle* h, double beta);

/* Filter-length constraint of the subband stream: with J > 0 every hop projects its per-bin filters, between the joint
 * diagonalisation and the output spectra, onto the spectra of causal J-tap impulse responses -- for every zone program that runs,
 * every rank index v and every loudspeaker l
 *   g = irfft(W[:, v, l], N)     (numpy's convention: the imaginary parts of bins 0 and N/2 are discarded)
 *   g[J:] = 0
 *   W'[:, v, l] = rfft(g, N)
 * and W' replaces W everywhere downstream: the output spectra and the synthesis use it, the states "w_A" / "w_B" hold it, and the
 * states "w_time_A" / "w_time_B" [nV][J][L] (float64 with cfg.out_c128, else float32) hold the taps g[:J] of the last hop: the
 * subband counterpart of the reference's J-tap w_A / w_B.  The target paths are a delta already and are not touched.  One more
 * kernel per hop (csrc/kernels_constrain.hip), part of the captured hop graphs; the taps buffers are allocated by apv_stream_init
 * only when J > 0.  apv_process_signal* on such a stream projects the filters of a chunk of 16 hops in one launch where its chunked
 * schedule applies (see there), else it runs its hops through the per-hop path.  J = 0 (the default) switches the
 * constraint off: the stream launches what it launches without this call, and has no "w_time_*" states.  Called between apv_create
 * and apv_stream_init; APV_ERR_ARG (nothing changed) once the stream is initialised or for J outside 0..block_size;
 * apv_stream_init refuses modeling_delay >= J (the reference puts its target tap at J ref + delay).
 *                                                         replaces: the J-tap filters of apvast.py:389-422 (filter_length) */
int  apv_stream_set_filter_taps(apv_handle* h, int32_t J);

/* The projection alone, without a stream: d_w [n_bins][nV][L] complex (c128 with cfg.out_c128, else c64), n_bins = N / 2 + 1,
 * projected in place onto J-tap responses as defined above, 1 <= J <= N; d_taps [nV][J][L] real of the same precision receives
 * g[:J] (NULL: not wanted).  Any even N the STFT accepts whose transform fits LDS in that precision.  On the handle's stream.
 *                                                         replaces: nothing in the reference (see apv_stream_set_filter_taps) */
int  apv_constrain_filters(apv_handle* h, void* d_w, int32_t n_bins, int32_t nV, int32_t L, int32_t N, int32_t J, void* d_taps);

/* Array-effort limit of the subband stream's filters.  The effort of output slot t of bin k is
 * e_t = sum_l |W[k, t, l]|^2; the target path is a unit filter on the reference loudspeaker, so e_t is the array effort relative
 * to that loudspeaker alone (1 = 0 dB).  With E = h_limit[z][k] (linear, > 0, +inf = no limit in that bin) every hop, behind the
 * joint diagonalisation and ahead of the filter-length projection, one more kernel (csrc/kernels_effort.hip) makes slot t
 *   unchanged                      if e_t <= E  (the slot is admissible; a non-finite e_t never is, and such a slot is left alone),
 *   a bit copy of slot t'          t' the largest admissible slot below t, if there is one,
 *   W[k, t, :] * sqrt(E / e_t)     otherwise (gain in float64, product rounded once to the filters' type).
 * e_t is summed in float64 in an order fixed by n_srcs.  Everything downstream (projection, taps, output spectra, FIR synthesis,
 * the states "w_A" / "w_B") sees the limited filters; eigenvalues, eigenvectors, statistics and the span's outputs do not change.
 * h_limit is [2][n_bins], row 0 = zone program A.  The first call allocates the table and the outputs and comes between apv_create
 * and apv_stream_init; later calls upload new values, which hold from the next hop on (the table is device memory: the captured
 * hop graphs stay).  A handle that never had a limit launches what it launched before.  APV_ERR_ARG, nothing changed: a value
 * that is NaN or <= 0, a first call on an initialised stream, a broadband handle.  The stage keeps no state from hop to hop.
 *                                                         replaces: nothing in the reference */
int  apv_stream_set_effort_limit(apv_handle* h, const double* h_limit);
/* Outputs of the effort limit of the last hop (after apv_process_signal*: of its last hop) for zone program `zone` (0 / 1), any of
 * them NULL when not wanted: h_effort [n_bins][n_ranks] float64 = the e_t before the stage; h_rank [n_bins] int32 = the rank (entry
 * of the rank list) of the slot the top slot was taken from, its own rank where it was scaled, 0 where its effort was not finite or
 * no hop has run; h_gain [n_bins] float64 = the gain of the top slot (1 unless scaled).  APV_ERR_ARG on a handle without a limit.
 * Synchronises the handle's stream. */
int  apv_get_effort(apv_handle* h, int32_t zone, double* h_effort, int32_t* h_rank, double* h_gain);
/* The stage alone, on host arrays: h_w [n_hops][K][nV][L] complex (c128 != 0: complex128, else complex64) limited in place by
 * h_limit [K] (the same table for every hop), nV <= 128; h_effort [n_hops][K][nV], h_rank [n_hops][K], h_gain [n_hops][K] as above
 * (may be NULL), except that h_rank is the INDEX of the source slot of the top slot (its own index where it was scaled, -1 where its
 * effort was not finite).  One launch, blockIdx.z = hop; every hop is computed as a call with that hop alone computes it. */
int  apv_limit_effort(apv_handle* h, int32_t c128, int32_t n_hops, int32_t K, int32_t nV, int32_t L, void* h_w, const double* h_limit,
                      double* h_effort, int32_t* h_rank, double* h_gain);

/* Rank choice per bin by the contrast at validation microphones.  The contrast is that of Matlab/main.m:120-130,
 * energy at the microphones of the program's own zone over energy at those of the other zone, predicted per bin from the static
 * transfer functions of the validation responses, G_z[k][m][l] = sum_j rv_z[j][l][m] exp(-2 pi i j k / N).  Per zone program, bin k
 * and output slot t (slots in ascending rank), in float64 whatever the filters' type:
 *   bright_t = sum_m |sum_l G_own[k][m][l] W[k][t][l]|^2,  dark_t = sum_m |sum_l G_other[k][m][l] W[k][t][l]|^2
 * (program A: own = zone A, other = zone B; program B the reverse).  With phi = h_floor[z][k] (linear, finite, >= 0) slot t' is
 * admissible if both energies are finite and bright >= phi dark.  Every hop, behind the joint diagonalisation (span included) and
 * ahead of the effort limit and the filter-length projection, one more kernel (csrc/kernels_valspan.hip) makes slot t a bit copy
 * of slot src_t: the largest admissible t' <= t; where there is none, the first t' <= t with finite energies that maximises
 * bright / dark (compared by cross-multiplication; dark = 0 < bright above every ratio, 0/0 lowest); where no slot t' <= t has
 * finite energies the slot is left as it is (src_t = -1).  phi = 0 is "no floor in this bin": the energies are reported and the
 * filters of the bin are not written.  Everything downstream sees the chosen filters; eigenvalues, eigenvectors, statistics and
 * the span's outputs do not change, and the stage keeps no state from hop to hop.
 * h_G_A / h_G_B are [n_bins][Mv][n_srcs] complex128 (Mv of apv_stream_set_evaluation), h_floor is [2][n_bins], row 0 = zone
 * program A.  The first call allocates the banks, the table and the outputs and comes after apv_stream_set_evaluation and before
 * apv_stream_init; later calls may pass NULL for both banks and then rewrite the floor alone.  New values hold from the next hop
 * on (device memory: the captured hop graphs stay).  A handle that never had the call launches what it launched before.
 * APV_ERR_ARG, nothing changed: a floor that is NaN, negative or infinite, a first call without the evaluation stage, without a
 * bank or on an initialised stream, one bank without the other, a broadband handle.
 *                                                         replaces: nothing in the reference */
int  apv_stream_set_validation_span(apv_handle* h, const void* h_G_A, const void* h_G_B, const double* h_floor);
/* Outputs of the stage of the last hop for zone program `zone` (0 / 1): what = APV_VALSPAN_BRIGHT / _DARK: [n_bins][n_ranks]
 * float64, the energies BEFORE the choice; _SOURCE: [n_bins][n_ranks] int32, src_t (-1: left as it is, or no hop has run);
 * _RANK: [n_bins] int32, the rank (entry of the rank list) of the top slot's source, 0 where it has none.  Synchronises the
 * handle's stream.  APV_ERR_ARG on a handle without the stage. */
enum { APV_VALSPAN_BRIGHT = 0, APV_VALSPAN_DARK = 1, APV_VALSPAN_SOURCE = 2, APV_VALSPAN_RANK = 3 };
int  apv_get_validation_span(apv_handle* h, int32_t zone, int32_t what, void* h_dst);
/* The stage alone for one program, on host arrays: h_w [K][nV][L] complex (c128 != 0: complex128, else complex64) replaced in
 * place; h_G_bright, h_G_dark [K][Mv][L] complex128; h_phi [K]; nV, L <= 128.  h_bright, h_dark [K][nV], h_src [K][nV] as above,
 * h_rank [K] = src of the top slot + 1 (the ranks being 1 .. nV; 0: none); any output may be NULL.  The call puts guard bands
 * around each of its device buffers and leaves in h_guard (may be NULL) the number of guard bytes the launch changed, and in h_ms
 * (may be NULL) the time of the launch alone between two events on the handle's stream, in milliseconds.  APV_ERR_ARG
 * with nothing launched: a null input, a size below 1, nV or L above 128, a floor that is not finite and >= 0. */
int  apv_validation_span(apv_handle* h, int32_t c128, int32_t K, int32_t nV, int32_t L, int32_t Mv, void* h_w, const void* h_G_bright,
                         const void* h_G_dark, const double* h_phi, double* h_bright, double* h_dark, int32_t* h_src, int32_t* h_rank,
                         int64_t* h_guard, float* h_ms);

/* Synthesis of the subband stream.  APV_SYNTH_WOLA (the default) is the reference's: output spectra, inverse transform, sine
 * window, overlap-add; its output lags the input by block_size - hop_size samples.  APV_SYNTH_FIR applies the J taps of a
 * constrained stream (apv_stream_set_filter_taps) as time-domain FIR filters with no latency: with x_z[n] the input of zone
 * program z at absolute sample n (zero before the first hop; input A feeds program A, input B program B), g_h the taps
 * "w_time_*" hold after hop h, g_{-1} = 0, and for hop h, t = 0 .. H - 1, n = h H + t, a_t = (t + 1) / H,
 *   y[z, v][n, l] = (1 - a_t) sum_{j < J} g_{h-1}[z, v, j, l] x_z[n - j]  +  a_t sum_{j < J} g_h[z, v, j, l] x_z[n - j]
 * -- a linear cross-fade over the hop from the previous hop's filter to this hop's -- and the target paths are the pure delays
 * x_A[n - modeling_delay] and x_B[n - modeling_delay] in the column of reference_index_A, zero in the others.  The results take
 * the places and the layout (cfg.out_layout) of the WOLA outputs; everything upstream of the synthesis, and every state and
 * attribute it leaves, is unchanged, bit for bit.  One launch per hop on the matrix cores plus a small one that moves the taps
 * and the history on (csrc/kernels_firsynth.hip), in the captured hop graphs; the output spectra and the inverse transform are
 * not launched, and "out_overlap" stays as it is.  States only such a stream has: "fir_synth_taps_A" / "fir_synth_taps_B"
 * [nV][J][L] in the filters' precision (the taps the next hop fades from; zone programs that run) and "fir_synth_history<g>"
 * [J - 1] in the sample precision (the newest samples of input signal g).  Called between apv_create and apv_stream_init;
 * APV_ERR_ARG (nothing changed) for an unknown mode or once the stream is initialised; apv_stream_init returns APV_ERR_ARG for
 * APV_SYNTH_FIR without filter taps.
 *                                                         replaces: nothing in the reference */
#define APV_SYNTH_WOLA 0
#define APV_SYNTH_FIR 1
int  apv_stream_set_synthesis(apv_handle* h, int32_t mode);

/* The synthesis kernel alone, on the handle's stream: d_x [J - 1 + H] samples of one signal (the J - 1 in front of the hop, then
 * the hop), d_taps_prev / d_taps_cur [nV][J][L], d_out [nV][H][L] as defined above.  Samples and results are float64 with a
 * float64 front-end (cfg.frontend / compute_dtype), else float32; taps float64 with cfg.out_c128, else float32.  APV_ERR_ARG for
 * J < 1, H < 1, nV < 1, L < 1, null pointers, or J beyond what the history window holds in LDS (about 8000 taps in float64).
 *                                                         replaces: nothing in the reference */
int  apv_fir_synthesis(apv_handle* h, const void* d_x, const void* d_taps_prev, const void* d_taps_cur, int32_t nV, int32_t L,
                       int32_t J, int32_t H, void* d_out);

/* Evaluation stage of the subband stream (off unless this is called): behind the synthesis of every hop, and in front of the copy
 * back, the device filters the hop's own drive signals through the responses to validation microphones, keeps the pressures of
 * the last hop, reduces them to energies per microphone and accumulates those (csrc/kernels_streameval.hip; two launches per hop,
 * part of the captured hop graphs).  h_rvA / h_rvB: float64 [Pv][L][Mv], L = cfg.n_srcs, the responses to the validation
 * microphones of zone A / zone B.  ranks: n_ranks rank values, strictly ascending, each in the handle's rank list: the evaluated
 * ranks, E of them.  Z = zone programs that run (cfg.n_zones), A first; "own" zone of program A is A.  Per absolute sample n, with
 * y zero before the first hop (lfilter with zero zi) and y_t the program's target output (A_t for program A, B_t for B):
 *   p_bright[z, v][n, m] = sum_l sum_{j < Pv} rv_own(z)  [j, l, m] y[z, v][n - j, l]
 *   p_dark  [z, v][n, m] = sum_l sum_{j < Pv} rv_other(z)[j, l, m] y[z, v][n - j, l]
 *   p_target[z][n, m]    = sum_l sum_{j < Pv} rv_own(z)  [j, l, m] y_t[z][n - j, l]
 * and per hop and microphone, summed over the hop's H samples in ascending order,
 *   bright = sum p_bright^2, dark = sum p_dark^2, error = sum (p_target - p_bright)^2, target = sum p_target^2.
 * All of it in float64 whatever the stream's precision (float32 samples are widened).  States only such a stream has
 * (apv_get_state / apv_set_state):
 *   "eval_pressure" f64 [Z][2 E + 1][H][Mv]: per program [bright of the E ranks][dark of the E ranks][target], last hop; read-only
 *   "eval_hops"     f64 [n][Z][3 E + 1][Mv]: per hop of the last apv_process_* call (n of them; apv_state_bytes tells) and program
 *                   [bright of the E ranks][dark ...][error ...][target]; read-only
 *   "eval_totals"   f64 [Z][3 E + 1][Mv]: the same summed over every hop since apv_stream_init or apv_stream_reset_evaluation,
 *                   total = total + hop, one addition per hop
 *   "eval_history"  [Z][E + 1][Pv - 1][L] in the sample precision: the newest Pv - 1 output samples of every evaluated group
 *                   (the E ranks, then the target), oldest first
 * apv_process_signal* on such a stream runs its hops one after the other through the per-hop path ("signal_schedule" {0, n}).
 * Called between apv_create and apv_stream_init.  APV_ERR_ARG (nothing changed) once the stream is initialised, for null pointers,
 * Pv < 1, Mv < 1, n_ranks outside 1..the handle's ranks, ranks not strictly ascending or not in the rank list, or Pv > 20465: one
 * loudspeaker's window of Pv - 1 + 16 float64 samples has to fit the 160 KB of LDS of a compute unit.  Mv up to 1048560.
 *                                                         replaces: Matlab/main.m:64-76, 120-130 with predictPressure.m:12-16 */
int  apv_stream_set_evaluation(apv_handle* h, int32_t Pv, int32_t Mv, const double* h_rvA, const double* h_rvB, int32_t n_ranks,
                               const int32_t* ranks);
/* "eval_totals" and both "eval_history" buffers to zero: the next hop's totals equal its own energies; with the per-bin spectra
 * on, "eval_spectra" and "eval_ring" too, and with the detectability stage "eval_detect".  APV_ERR_ARG without such a stream. */
int  apv_stream_reset_evaluation(apv_handle* h);
/* Per-bin spectra of the evaluation stage (off unless called with on = 1; needs apv_stream_set_evaluation): behind the two launches
 * of the evaluation stage the device keeps the last N = block_size pressure samples of every pressure set and microphone in a
 * ring, and after every hop transforms the newest N of them under the stream's analysis window and accumulates the squared
 * magnitudes per bin (csrc/kernels_evalspec.hip; three more launches per hop, part of the captured hop graphs).  With H the hop,
 * K = N/2 + 1, w[i] = sin(pi i / N), hop t counted from apv_stream_init, a set "eval_ring" or apv_stream_reset_evaluation
 * (t = 0 first), and p as defined above, zero before sample 0:
 *   f_t[s][i, m] = p[s][(t + 1) H - N + i, m], i < N        P_t[s][k, m] = sum_i w[i] f_t[s][i, m] exp(-2 pi i k i / N), k < K
 *   bright[z, v, m, k] += |P_bright|^2, dark += |P_dark|^2, error += |P_target - P_bright|^2, target[z, m, k] += |P_target|^2
 * -- one addition per element and hop, no atomics, float64 whatever the stream's precision.  States only such a stream has:
 *   "eval_spectra"  f64 [Z][3 E + 1][K][Mv]: per program [bright of the E ranks][dark ...][error ...][target], bins before
 *                   microphones (the order the device accumulates in), summed since apv_stream_init or the last reset
 *   "eval_ring"     f64 [Z (2 E + 1)][Mv][N]: the last N pressure samples per set (the order of "eval_pressure") and microphone,
 *                   oldest first
 * apv_stream_reset_evaluation zeroes both.  Called between apv_create and apv_stream_init; APV_ERR_ARG (nothing changed) once the
 * stream is initialised or for a value other than 0 and 1.  apv_stream_init returns APV_ERR_ARG when it is on without
 * apv_stream_set_evaluation, and for block_size > 4096: the float64 transforms in LDS stop there, so a float32 stream with a
 * larger block cannot have the spectra.                     replaces: nothing in the reference (pwelch on the host) */
int  apv_stream_set_evaluation_spectra(apv_handle* h, int32_t on);
/* One step of that stage alone, on device pointers and the handle's stream: d_pressure [Z (2 E + 1)][H][Mv] goes into the ring
 * d_ring [Z (2 E + 1)][Mv][N] behind the offset ring_off -- logical sample n of a row lives at (n + ring_off) mod N, the hop
 * takes the logical samples N - H .. N - 1; a caller stepping through hops advances ring_off by H mod N BEFORE each call, as the
 * stream does -- every row is windowed and transformed, and |P|^2 is added to d_totals [Z][3 E + 1][N/2 + 1][Mv].  All float64.
 * The call allocates and frees the transform's scratch and synchronises.  APV_ERR_ARG for null pointers, sizes below 1, odd N,
 * N > 4096, Z > 2, H > N or ring_off outside 0..N - 1.       replaces: nothing in the reference */
int  apv_eval_spectrum_step(apv_handle* h, const double* d_pressure, double* d_ring, int32_t ring_off, int32_t N, int32_t H, int32_t Z,
                            int32_t E, int32_t Mv, double* d_totals);
/* Perceptual detectability of the evaluated pressures (off unless called with n_channels > 0; needs the per-bin spectra): behind
 * the launches of the spectra stage three more (csrc/kernels_evaldetect.hip, part of the captured hop graphs) evaluate the second
 * half of the masking model, evaluateDetectability, on the hop's spectra P_t.  With f = 2 / N^2, G2 [K][C] the model's squared
 * channel responses, and the squared weighting curve of a masker spectrum S
 *   w2_S[k] = Cs Leff sum_c G2[k, c] / (f sum_j G2[j, c] |S[j]|^2 + Ca)                       (the masker includes bin 0)
 * per hop, program z, evaluated rank e and validation microphone m, T the target, B the bright and Dk the dark spectrum:
 *   error[z, e, m] = sum_{k >= 1} w2_{T[z, m]}[k] f |T[z, m, k] - B[z, e, m, k]|^2            the reproduction error, masked by the
 *                                                                                             programme the listener wants
 *   leak [z, e, m] = sum_{k >= 1} w2_{T[1 - z, m]}[k] f |Dk[z, e, m, k]|^2                    the other programme's leakage, masked
 *                                                                                             by that zone's own target
 * -- D = 1 is just audible; with one program (Z = 1) the leak's masker is silence, the threshold in quiet.  float64 whatever the
 * stream's precision, no atomics.  States only such a stream has:
 *   "eval_detect"       f64 [Z][6 E][Mv]: per program [sum | max | number of hops with D > 1] of the error of the E ranks, then the
 *                       same three of the leak, since apv_stream_init or the last reset (total = total + hop per hop)
 *   "eval_detect_hops"  f64 [hops of the last call][Z][2 E][Mv], read-only: per program the error of the E ranks, then the leak
 * apv_stream_reset_evaluation zeroes "eval_detect".  h_G2 [n_bins][n_channels], Cs, Ca, Leff: the tables of the model
 * (perceptual.PerceptualTables).  Called between apv_create and apv_stream_init; n_channels = 0 switches the stage off.
 * APV_ERR_ARG (nothing changed) once the stream is initialised, for n_channels outside 0..512, a null table, a non-finite table
 * entry or constant, or Ca <= 0.  apv_stream_init returns APV_ERR_ARG when the stage is on without
 * apv_stream_set_evaluation_spectra.                     replaces: Matlab/ControlMethods/perceptualModel.m:192-206, on the device */
int  apv_stream_set_evaluation_detectability(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff);
/* One step of that stage alone, on device pointers and the handle's stream: d_spec [N/2 + 1][Z (2 E + 1) Mv] complex128, the
 * bin-major spectra of the pressure sets (per program: bright of the E ranks, dark of the E ranks, target); h_G2 [N/2 + 1][n_channels]
 * on the host.  The hop's values go to d_hop [Z][2 E][Mv] and into d_totals [Z][6 E][Mv] as above.  The call uploads the tables,
 * allocates and frees its scratch and synchronises.  APV_ERR_ARG for null pointers, sizes below 1, odd N, Z > 2, n_channels > 512,
 * non-finite constants, Ca <= 0 or a block the curve kernel's LDS does not hold (N/2 + 1 + n_channels > 8192).
 *                                                        replaces: nothing in the reference */
int  apv_eval_detect_step(apv_handle* h, const void* d_spec, int32_t N, int32_t Z, int32_t E, int32_t Mv, int32_t n_channels,
                          const double* h_G2, double Cs, double Ca, double Leff, double* d_hop, double* d_totals);
/* The pressure kernel alone, on the handle's stream: d_y [G][Pv - 1 + H][L] samples (per group the Pv - 1 in front of the hop,
 * then the hop; float64 with a float64 front-end, else float32), d_rv [Pv][L][Mv] float64, d_p [G][H][Mv] float64:
 * p[g][n, m] = sum_l sum_j rv[j, l, m] y[g][Pv - 1 + n - j, l].  APV_ERR_ARG for a size below 1, null pointers, G > 65535 or
 * Pv > 20465.                                             replaces: Matlab/predictPressure.m:12-16 */
int  apv_eval_pressure(apv_handle* h, const void* d_y, const double* d_rv, int32_t G, int32_t L, int32_t Pv, int32_t H, int32_t Mv,
                       double* d_p);
/* The energy reduction of the broadband stream's evaluation stage alone, on the handle's stream: d_p [Z][2 E + 1][n_hops H][Mv]
 * float64 pressures (per program: bright of the E ranks, dark of the E ranks, target) of n_hops consecutive hops -> d_record
 * [n_hops][Z][3 E + 1][Mv], per hop bright = sum p_bright^2, dark = sum p_dark^2, error = sum (p_target - p_bright)^2 per rank and
 * target = sum p_target^2 over the hop's H samples, summed in an order that depends on H alone; then d_totals [Z][3 E + 1][Mv]
 * <- d_totals + d_record[i], i ascending.  No atomics.  APV_ERR_ARG for null pointers, Z outside 1..2, another size below 1, or
 * n_hops x H of 2^31 and more.                            replaces: Matlab/main.m:120-130, the sums */
int  apv_eval_energies(apv_handle* h, const double* d_p, int32_t Z, int32_t E, int32_t H, int32_t Mv, int32_t n_hops, double* d_record,
                       double* d_totals);
/* The three launches of apv_bb_set_evaluation_spectra alone, on device pointers and the handle's stream: d_pressure
 * [Z (2 E + 1)][n_hops H][Mv], the pressures of n_hops consecutive hops; d_tail [Z (2 E + 1)][Mv][N - H], in and out, the newest
 * N - H samples in front of the first hop and behind the last, oldest first (may be null when H = N); |P|^2 of every hop's frame
 * is added to d_totals [Z][3 E + 1][N/2 + 1][Mv] in hop order.  hops_per_launch = 0: sub-launches of as many hops as the scratch
 * budget allows; otherwise of at most that many, through the same loop the stream runs -- the totals' bits do not depend on it.
 * All float64.  The call allocates and frees its lines and scratch and synchronises.  APV_ERR_ARG for null pointers, sizes below
 * 1, odd N, N > 4096, H > N, Z > 2, hops_per_launch < 0, or n_hops x H of 2^31 and more.
 *                                                         replaces: nothing in the reference */
int  apv_eval_spectra_hops(apv_handle* h, const double* d_pressure, double* d_tail, int32_t N, int32_t H, int32_t Z, int32_t E,
                           int32_t Mv, int32_t n_hops, int32_t hops_per_launch, double* d_totals);
/* The three hop-batched launches of apv_bb_set_evaluation_detectability alone, on device pointers and the handle's stream: d_spec
 * [n_hops][N/2 + 1][Z (2 E + 1) Mv] complex128, the bin-major spectra of n_hops consecutive hops (per program: bright of the E
 * ranks, dark of the E ranks, target); h_G2 [N/2 + 1][n_channels] on the host.  Hop i's values go to d_hops [n_hops][Z][2 E][Mv]
 * and, in hop order, into d_totals [Z][6 E][Mv] as for apv_eval_detect_step, whose bits a call with one hop reproduces.  The hops
 * run as sub-launches of at most hops_per_launch, through the same loop the stream runs -- no bit depends on it.  The call uploads
 * the tables, allocates and frees its scratch and synchronises.  APV_ERR_ARG (outputs untouched) for null pointers, sizes below 1,
 * hops_per_launch < 1, odd N, Z > 2, n_channels > 512, non-finite constants, Ca <= 0 or N/2 + 1 + n_channels > 8192.
 *                                                         replaces: nothing in the reference */
int  apv_eval_detect_hops(apv_handle* h, const void* d_spec, int32_t n_hops, int32_t hops_per_launch, int32_t N, int32_t Z, int32_t E,
                          int32_t Mv, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff, double* d_hops,
                          double* d_totals);

/* ---- device memory / stream plumbing ----------------------------------- */
int  apv_dev_alloc(apv_handle* h, size_t bytes, void** d_ptr);
int  apv_dev_free(apv_handle* h, void* d_ptr);
int  apv_memcpy_h2d(apv_handle* h, void* d_dst, const void* h_src, size_t bytes);   /* async on the handle's stream */
int  apv_memcpy_d2h(apv_handle* h, void* h_dst, const void* d_src, size_t bytes);   /* async on the handle's stream */
int  apv_sync(apv_handle* h);                                  /* hipStreamSynchronize */
/* HIP-event timer on the handle's stream (bench.py's roofline leg) */
int  apv_timer_start(apv_handle* h);
int  apv_timer_stop(apv_handle* h, float* elapsed_ms);         /* synchronises on the stop event */

/* ---- the hot path, device-resident ------------------------------------- */
/* One block of subband filter updates: for each owned bin k
 *   R_B = X_B^H X_B, R_D = X_D^H X_D, r = X_B^H d          replaces apvast.py:329-364 (update_statistics)
 *   U, lam = jdiag(R_B, R_D)                                replaces apvast.py:20-36, 378-387
 *   w_V = sum_{i<V} (u_i^H r)/(lam_i+mu) u_i                replaces apvast.py:406-414
 * R, U never touch HBM.  d_lam / d_status may be NULL.
 */
int  apv_update_dev(apv_handle* h, const void* d_XB, const void* d_XD, const void* d_d,
                    void* d_w, void* d_lam, int32_t* d_status);

/* Pipelining of consecutive apv_update_dev calls (the caller of apvast.py:153-165 runs one block after the other; blocks of
 * different streams or hops are independent).  n = 2: launches alternate between two streams of the handle's, so that the last
 * waves of one launch finish beside the first waves of the next (+6 % updates/s at BASELINE config 2).  Results are those of
 * n = 1 bit for bit.  Ordering stays the library's business: a launch whose operands overlap the other lane's launch in flight
 * (same output buffer, an input that the other writes) waits for it; copies, timers, apv_sync, apv_update and the all-gather see
 * every launch queued before them; launches queued after a copy see the copy.  Orders 33..64 park per-bin state in scratch slots:
 * the second stream gets slots of its own (allocated by this call: the per-block path still allocates nothing); the split float32
 * update (orders 32 / 64 in APV_F32) shares one scratch matrix and keeps to one stream.  n = 1 (the default): every launch on the
 * handle's stream. */
int  apv_set_update_streams(apv_handle* h, int32_t n);

/* Same from caller-owned host buffers (copies in, runs, copies out, syncs). */
int  apv_update(apv_handle* h, const float* h_XB, const float* h_XD, const float* h_d,
                void* h_w, void* h_lam, int32_t* h_status);

/* K5': correlation only -> R_B, R_D [K][L][L], r [K][L] in the compute dtype
 * (c64 for APV_F32, c128 for APV_F64), device-resident.   replaces apvast.py:329-364
 * n_srcs <= 64: APV_ERR_ARG on a handle of a larger order. */
int  apv_corr_dev(apv_handle* h, const void* d_XB, const void* d_XD, const void* d_d,
                  void* d_RB, void* d_RD, void* d_r);

/* The same contraction from bf16 inputs ((re, im) bf16 pairs, 4 bytes per element, same [K][M][L] layout), f32
 * accumulation on the bf16 matrix cores; R_B, R_D [K][L][L] and r [K][L] come out as c64.  n_srcs in {32, 64}.
 * (BASELINE config 5: fp32 vs bf16 correlation accumulation.)  apv_to_bf16_dev converts `count` c64 elements. */
int  apv_corr_bf16_dev(apv_handle* h, const void* d_XB, const void* d_XD, const void* d_d,
                       void* d_RB, void* d_RD, void* d_r);
int  apv_to_bf16_dev(apv_handle* h, size_t count, const void* d_c64, void* d_bf16);

/* K6-K10: GEVD + filter from explicit R_B, R_D, r (compute dtype).   replaces apvast.py:378-414 */
int  apv_gevd_vast_dev(apv_handle* h, const void* d_RB, const void* d_RD, const void* d_r,
                       void* d_w, void* d_lam, int32_t* d_status);

/* Module-level jdiag drop-in (apvast.py:20-36), batched: `batch` pairs of n x n Hermitian
 * (A, B) in c128 (row-major), B loaded with reg per the handle's reg_mode/reg_dark.
 * U: [batch][n][n] c128 (columns = eigenvectors, descending), lam: [batch][n] f64.
 * Host buffers. n <= APV_MAX_N. */
int  apv_jdiag_batched(apv_handle* h, int32_t n, int32_t batch, const double* h_A, const double* h_B,
                       double* h_U, double* h_lam, int32_t* h_status);

/* The same for REAL symmetric pairs of broadband order (n = filter_length x loudspeakers: 256 at cfg1, 800 with
 * the parameters of make_python_test.m, 4000 with those of main.m), n <= 4096: A, B, U are [batch][n][n] f64 row-major, lam [batch][n].
 * Matrices live in HBM; one launch per elimination step and per Jacobi round.   replaces apvast.py:20-36 at
 * the sizes of its call sites apvast.py:380, 382 */
int  apv_jdiag_large(apv_handle* h, int32_t n, int32_t batch, const double* h_A, const double* h_B,
                     double* h_U, double* h_lam, int32_t* h_status);
/* The leading `rank` eigenpairs of real symmetric pairs of broadband order -- what the filters consume: apvast.py:406-414 uses
 * U[:, :V] and diag(D)[:V] of the jdiag call at apvast.py:380, 382.  U: [batch][n][rank] (columns = eigenvectors, descending,
 * U^T (B + reg I) U = I), lam: [batch][rank].  Chebyshev-filtered subspace iteration on the whitened matrix
 * (kernels_gevd_lead.hip); h_info[z] = 0: that solver converged, 1: the call fell back to the complete block-Jacobi solve of
 * apv_jdiag_large (flat spectrum beyond the cut, rank too large for a block of 64, Gram breakdown) -- the results are
 * valid either way.  h_info may be NULL.                      replaces apvast.py:20-36 + the slices of 406-414 */
int  apv_jdiag_leading(apv_handle* h, int32_t n, int32_t batch, int32_t rank, const double* h_A, const double* h_B,
                       double* h_U, double* h_lam, int32_t* h_info);
/* Complex Hermitian pairs beyond the per-bin orders, n <= 1024 (apvast.py:20-36 takes any order; apv_jdiag_batched stops at
 * 64): A, B, U are [batch][n][n] complex128 row-major, lam [batch][n] f64.  Runs the real symmetric solver above on the
 * embedding [Re -Im; Im Re] of order 2n and keeps n of its 2n eigenvectors that are independent over C
 * (kernels_jdiag_cplx.hip).  status 3 / APV_ERR_NO_CONVERGE: an eigenvalue cluster of ~40 or more coincident values.
 *                                                         replaces apvast.py:20-36 */
int  apv_jdiag_large_c128(apv_handle* h, int32_t n, int32_t batch, const void* h_A, const void* h_B,
                          void* h_U, double* h_lam, int32_t* h_status);
/* h_out[i] = ||M_i||_2 for `count` symmetric positive semi-definite n x n matrices h_mats [count][n][n] f64 (host), n <= 4096:
 * the largest Ritz value of 96 Lanczos steps, the norm of the relative loading apVast.m:552-569 (apv_bb_set_rank_list) and
 * of apv_jdiag_* with APV_REG_REL.  method: APV_NORM2_AUTO is what those paths run -- one workgroup per matrix up to
 * n = 2048, above that every step's matrix-vector product spread over the chip; APV_NORM2_ONE_WG / APV_NORM2_GRID force one
 * of the two.                                              replaces norm(R) of apVast.m:559-566 */
#define APV_NORM2_AUTO   0
#define APV_NORM2_ONE_WG 1
#define APV_NORM2_GRID   2
int  apv_norm2(apv_handle* h, int32_t n, int32_t count, const double* h_mats, double* h_out, int32_t method);

/* ---- STFT stages (K2-K4) ------------------------------------------------ */
/* spectra[c][k] = rfft(window * x[c][:])  for `n_ch` channels of length N (f32 in, c64 out,
 * both channel-major, device).      replaces apvast.py:202-203, 246-255, 430-431 */
int  apv_stft_analysis_dev(apv_handle* h, int32_t n_ch, const float* d_x, void* d_spec);
/* overlap[c] = shift(overlap[c], H) + window * irfft(spec[c]); out[c][0:H] = overlap[c][0:H].
 *                                   replaces apvast.py:212-225, 265-293, 457-504 */
int  apv_istft_ola_dev(apv_handle* h, int32_t n_ch, const void* d_spec, float* d_overlap, float* d_out);
/* The transforms as the streams launch them, on their own (block and hop size from the handle's config; f64 = 0: float / c64
 * data, 1: double / c128; every pointer is device memory).
 * Analysis: spec[c * stride_c + k * stride_k] = rfft(w * y_c)[k], k <= N/2, with y_c[n] = x[c * x_stride + (n + ring_off) mod N]
 * for n < in_len and 0 for in_len <= n < N; w the sine window (use_win = 1) or all ones (use_win = 0).  APV_ERR_ARG unless
 * 0 <= in_len <= N and x_stride >= in_len; a non-zero ring_off (any sign, taken modulo N) needs in_len == N and x_stride >= N;
 * f64 needs N <= 4096.                                  apvast.py:246-255, 417-422, 430-431 */
int  apv_analysis_dev(apv_handle* h, int32_t f64, int32_t n_ch, const void* d_x, int64_t x_stride, int32_t in_len,
                      int32_t ring_off, int32_t use_win, void* d_spec, int64_t stride_c, int64_t stride_k);
/* Windowed full-length analysis of n_jobs (1..8) channel sets in ONE launch, the form a streaming hop runs: set j has n_ch[j]
 * channels at d_x[j] and writes spec[j][c * stride_c[j] + k * stride_k[j]].  A set whose stride_c and stride_k both exceed 1 is
 * GROUPED: g = stride_c[j] neighbouring bins of a channel are contiguous, element (c, k) at (k / g) * g * stride_k[j] + c * g + k % g.
 * n_hops = 0: one hop, rows of N samples read as rings at ring_off.  n_hops in 1..65535: the chunk form, rows x_stride >= N +
 * (n_hops - 1) * x_hop samples apart, hop i reads its block i * x_hop samples into the row and writes spec_hop[j] * i elements
 * further on (ring_off must be 0). */
int  apv_analysis_jobs_dev(apv_handle* h, int32_t f64, int32_t n_jobs, const void* const* d_x, const int32_t* n_ch,
                           void* const* d_spec, const int64_t* stride_c, const int64_t* stride_k, int32_t ring_off,
                           int32_t n_hops, int64_t x_stride, int64_t x_hop, const int64_t* spec_hop);
/* Synthesis + overlap-add: new = w * irfft(spec_c) (imaginary parts of DC and Nyquist ignored), overlap[c] (N samples, channel-
 * major) = shift(overlap[c], H) + new, and, unless d_out is NULL, out = overlap[c][0:H]: channel-major [n_ch][H], or with
 * out_group > 0 dividing n_ch sample-major in groups [n_ch / out_group][H][out_group], the groups out_gstride elements apart
 * (0: H * out_group; otherwise at least that).  An out_group that does not divide n_ch emits channel-major.
 *                                                         apvast.py:265-293, 457-504 */
int  apv_synthesis_dev(apv_handle* h, int32_t f64, int32_t n_ch, const void* d_spec, int64_t stride_c, int64_t stride_k,
                       void* d_overlap, void* d_out, int32_t out_group, int64_t out_gstride);

/* ---- streaming composition (one call = one hop) -------------------------- */
/* Upload the room impulse responses and allocate all streaming state.  h_rir_A / h_rir_B: (rir_len, L, M)
 * float64, C order -- exactly what scipy.io.loadmat('rirs.mat') gives after np.ascontiguousarray
 * (make_python_test.m:4,18).  The handle must have been created with block_size, hop_size,
 * n_bins = block_size/2+1 and n_zones = bit mask (1 = zone A, 2 = zone B: run_A/run_B, apvast.py:53-54).
 *                                                         replaces apvast.__init__, apvast.py:97-151 */
int  apv_stream_init(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B,
                     int32_t reference_index_A, int32_t reference_index_B, int32_t modeling_delay);
/* One hop of both input signals (H float32 samples each).  h_out: [n_out][H] float32 with channels
 * [zone A: nV x L][zone B: nV x L] (zones that run) followed by [A_t: L][B_t: L]  (cfg.out_layout = 1: the same groups of L
 * channels, each written [H][L]).
 *                                                         replaces process_input_buffers, apvast.py:153-165 */
int  apv_process_block(apv_handle* h, const float* h_in_A, const float* h_in_B, float* h_out);
/* The same with float64 samples on the host side (lossless with the float64 front-end; either entry point works
 * with either front-end, converting on the host).  A hop in which some bin reached the Jacobi sweep cap returns
 * APV_ERR_NO_CONVERGE after h_out has been written.      replaces process_input_buffers, apvast.py:153-165 */
int  apv_process_block_f64(apv_handle* h, const double* h_in_A, const double* h_in_B, double* h_out);
/* n_hops consecutive hops in one call: h_in_A / h_in_B hold n_hops * H samples, h_out is [n_hops][n_out][H] with the
 * channel order of apv_process_block.  Sample for sample the result is that of n_hops calls of apv_process_block (same
 * kernels, same operands, same order within a hop); the hops are pipelined: RIR convolution + analysis of hop h+1 run on a second
 * stream beside the joint diagonalisation of hop h, synthesis and copy back on a third, and the host stages / converts
 * one chunk of 16 hops while the device runs the next.  A hop with a bin that is not positive definite returns APV_ERR_NOT_PD once the
 * chunks in flight (its own and at most one more) have run (the message names the hop; the stream's state is then that
 * after the last hop run); APV_ERR_NO_CONVERGE is returned after all hops, every output written.  With responses of 64 taps or
 * more (K1 in one fast-convolution segment) and no statistics window or forgetting, a chunk of 16 hops is a handful of launches:
 * the front halves, and for a constrained stream the projection and the FIR synthesis, one launch per chunk each.  The read-only
 * state "signal_schedule", two int32, tells which way the last call went: {hops through chunk launches, hops hop by hop};
 * {0, 0} before the first call, and apv_process_block* does not touch it.
 *                        replaces the hop loop around processInputBuffer, main.m:52-62 / make_python_test.m:44-51 */
int  apv_process_signal(apv_handle* h, int32_t n_hops, const float* h_in_A, const float* h_in_B, float* h_out);
int  apv_process_signal_f64(apv_handle* h, int32_t n_hops, const double* h_in_A, const double* h_in_B, double* h_out);
/* 1 if the stream's front-end (and therefore its named state arrays) is float64, 0 if float32, -1 without a stream */
int  apv_stream_is_f64(apv_handle* h);
/* Per-bin statistics and eigenvectors of the CURRENT hop of a streaming handle, recomputed in float64 on demand from
 * the hop's control-point spectra (the per-hop path never writes R or U to HBM).  zone 0 = A (bright A->A, dark A->B),
 * 1 = B.  h_RB, h_RD, h_U [K][L][L] c128 (U: columns = eigenvectors, descending), h_r [K][L] c128, h_lam [K][L] f64; any
 * of them may be NULL.       replaces the attributes R_*, r_*, U_*, lambda_* of apvast.py:368-387, per bin */
int  apv_stream_get_statistics(apv_handle* h, int32_t zone, double* h_RB, double* h_RD, double* h_r, double* h_U,
                               double* h_lam);
/* hops so far (either stream mode) in which some bin reached the Jacobi sweep cap; each such hop also returned
 * APV_ERR_NO_CONVERGE with its outputs written and the stream advanced: a warning to the caller, not a lost hop */
long apv_stream_not_converged(apv_handle* h);
/* Perceptual ("AP") weighting of the control-point and target spectra, evaluated per block on the device from the
 * target spectra (van de Par 2005 model as carried by the reference's MATLAB twin).  h_G2 [K][n_channels] float64
 * = squared outer/middle-ear x gammatone responses; n_channels = 0 switches it off (all-ones, apvast.py:326-327).
 *                         replaces update_perceptual_weighting, apvast.py:313-324 / apVast.m:386-408 */
int  apv_stream_set_perceptual(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca,
                               double Leff, int32_t normalisation);
/* New room responses between two hops, without tearing the stream down.  h_rir_A / h_rir_B: (rir_len, L, M), h_trir_A /
 * h_trir_B: (rir_len, M) target responses, all float64 C order; NULL = that response is unchanged (targets are not re-derived from
 * new rir_*: the reference builds them once, apvast.py:100-112).  rir_len must equal the stream's (else APV_ERR_ARG, nothing
 * changed).  Every sample that arrived before the call keeps ringing out through the response it was filtered with, the samples
 * of the next hop on go through the new one: the difference is added to the next ceil((rir_len - 1) / H) hops as a correction tail
 * (state "fir_correction<p>" [C][rir_len-1], "target_fir_correction<z>" [M][rir_len-1]).  Several calls compose.
 *                        replaces `ap.rir_A = ...` etc. between two hops, read by lfilter(..., zi=state) at apvast.py:167-193 */
int  apv_stream_set_rirs(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B, const double* h_trir_A,
                         const double* h_trir_B);
/* mu of the next hop on, either stream mode (the subband stream's captured per-hop graphs are captured again).
 *                        replaces `ap.mu = ...` between two hops, read at apvast.py:161, 406-414 */
int  apv_set_mu(apv_handle* h, double mu);
/* The per-bin span of the subband filters.  With lambda_1 >= ... >= lambda_L, u_i the sorted joint eigenvectors of
 * bin k of zone program z and a_i = (u_i^H r) / (lambda_i + mu_k):
 *   h_mu_profile [2][n_bins] (>= 0, finite)  mu_k = cfg.mu * profile[z][k]
 *   h_rank_cap   [2][n_bins] (1..n_srcs)     no output slot of the bin goes past rank cap[z][k]
 *   contrast_floor phi (> 0; 0 = none)       ... nor past f_k, the number of leading v for which
 *                                            sum_{i<=v} lambda_i |a_i|^2 >= phi sum_{i<=v} |a_i|^2   (at least 1)
 * Output slot t of the bin holds the filter of rank min(ranks[t], cap, f_k); lambda is unchanged.  Row 0 of a table is zone
 * program A and every kernel-level call (apv_update*, apv_gevd_vast_dev), row 1 program B.  NULL / 0: that part is absent.
 * The first call fixes which parts exist; for a stream it precedes apv_stream_init.  Later calls change the values of the parts
 * that exist, from the next launch or hop on (tables are uploaded on the handle's stream; for phi the per-hop graphs of a stream
 * are captured again).  APV_ERR_ARG, with nothing changed: a part added or removed later, a negative or non-finite profile, a cap
 * outside 1..n_srcs, phi < 0 or non-finite, a handle with two update streams.  apv_set_mu on such a handle re-forms cfg.mu *
 * profile.  The broadband entry points refuse a handle with a span.           replaces: nothing in the reference */
int  apv_set_span(apv_handle* h, const double* h_mu_profile, const int32_t* h_rank_cap, double contrast_floor);
/* Outputs of the span of the last launch (after apv_process_signal*: of its last hop) for zone program `zone` (0 / 1):
 * h_rank [n_bins] int32 = min(last rank of the list, cap, f_k), 0 in a bin of status 1; h_contrast [n_bins][n_srcs] float64 (may be
 * NULL) = the contrast curve c_v = sum_{i<=v} lambda_i |a_i|^2 / sum_{i<=v} |a_i|^2.  APV_ERR_ARG on a handle without a span and
 * when h_contrast is asked for without a floor.  Synchronises the handle's stream. */
int  apv_get_span(apv_handle* h, int32_t zone, int32_t* h_rank, double* h_contrast);
/* Named state arrays for fixtures / checkpoint-resume (names: see stream.hip), in the front-end precision:
 * float32 / complex64, or float64 / complex128 with the float64 front-end.          apvast.py:115-151 */
int  apv_state_bytes(apv_handle* h, const char* name, size_t* bytes);
int  apv_get_state(apv_handle* h, const char* name, void* h_dst, size_t bytes);
int  apv_set_state(apv_handle* h, const char* name, const void* h_src, size_t bytes);

/* ---- broadband (time-domain) mode: the reference's own algorithm, float64 ---------------------------- */
/* Rank list of the next apv_bb_init: apVast.m:527-549 takes a vector of ranks and emits one solution per entry
 * (ascending, each 1..J L); n_ranks = 0 restores "every rank 1..number_of_eigenvectors" (apvast.py:406-422).
 * With cfg.dialect = APV_DIALECT_MATLAB the stream also follows apVast.m:410-456 (contiguous data matrix, R and r
 * divided by (S-J+1) M), apVast.m:597-602 (one target reference per zone) and, with cfg.reg_mode = APV_REG_REL,
 * apVast.m:552-569 (bright += reg_bright ||R||_2, dark += reg_dark ||R||_2 in place; spectral norm = largest Ritz
 * value of 96 Lanczos steps). */
int  apv_bb_set_rank_list(apv_handle* h, int32_t n_ranks, const int32_t* ranks);
/* One real (J L) x (J L) pair per zone per hop from `statistics_buffer_length` samples, J-tap filters, every rank
 * 1..V (apvast.py:329-422) or the registered rank list.  The handle needs block_size, hop_size, n_srcs, n_mics,
 * n_zones, mu, dialect, reg_mode and reg_dark (reg_mode = APV_REG_ABS: dark + reg_dark I inside the joint
 * diagonalisation, apvast.py:22-24; APV_REG_REL: see above); n_bins / ranks are not used.  J L <= 4096,
 * block_size <= 4096.  A failed factorisation (APV_ERR_NOT_PD) leaves the input/response/statistics buffers
 * advanced by the hop and the output overlap buffers untouched.
 *                                                         replaces apvast.__init__, apvast.py:40-151 */
int  apv_bb_init(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B,
                 int32_t reference_index_A, int32_t reference_index_B, int32_t modeling_delay,
                 int32_t filter_length, int32_t statistics_buffer_length, int32_t number_of_eigenvectors);
/* One hop (H float64 samples per signal).  h_out: [n_out][H] float64, channels as for apv_process_block with
 * nV = the number of ranks kept; with cfg.out_layout = 1: [n_out / L][H][L], one (hop, loudspeaker) array per zone program
 * and rank as process_input_buffers returns them (apvast.py:498-504).   replaces process_input_buffers, apvast.py:153-165 */
int  apv_bb_process_block(apv_handle* h, const double* h_in_A, const double* h_in_B, double* h_out);
/* n_hops consecutive hops in one call: h_in_A / h_in_B hold n_hops * H samples, h_out is [n_hops][n_out][H] with the channel
 * order of apv_bb_process_block -- with cfg.out_layout = 1: [n_out / L][n_hops * H][L], every group's whole signal as one
 * (sample, loudspeaker) array.  Each group of hops reaches the host in one copy: by DMA into a page-locked h_out
 * (apv_host_alloc), else through a staging set that the host empties while the device works on the next group.  A hop's statistics never depend on an earlier hop's filters, so the joint diagonalisations
 * of up to 16 consecutive hops (8 at large orders) are solved as ONE batch (the dependent launches of a single n = 256 pair leave most of the chip
 * idle); rings, overlap buffers and outputs advance hop by hop as in the per-hop call.  Outputs equal those of n_hops calls
 * of apv_bb_process_block up to the rounding of the eigen-iteration (a batch sweeps until its slowest member has converged).
 *                        replaces the hop loop of main.m:52-62 / make_python_test.m:44-51 around apvast.py:153-165 */
int  apv_bb_process_signal(apv_handle* h, int32_t n_hops, const double* h_in_A, const double* h_in_B, double* h_out);
/* Page-locked host memory for result arrays (hipHostMalloc, visible to every device): device-to-host copies into it are
 * asynchronous DMA transfers.  No reference counterpart (numpy allocates the reference's results, apvast.py:433-443). */
int  apv_host_alloc(void** p, size_t bytes);
int  apv_host_free(void* p);
/* perceptual weighting for the broadband stream; arguments as for apv_stream_set_perceptual */
int  apv_bb_set_perceptual(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff,
                           int32_t normalisation);
/* apv_stream_set_rirs for the broadband stream (same arguments and semantics).
 *                        replaces `ap.rir_A = ...` etc. between two hops, read by lfilter(..., zi=state) at apvast.py:167-193 */
int  apv_bb_set_rirs(apv_handle* h, int32_t rir_len, const double* h_rir_A, const double* h_rir_B, const double* h_trir_A,
                     const double* h_trir_B);
/* float64 state arrays by name (stream_bb.hip); `count` = number of doubles */
int  apv_bb_get_state(apv_handle* h, const char* name, double* h_dst, size_t count);
int  apv_bb_set_state(apv_handle* h, const char* name, const double* h_src, size_t count);
/* Evaluation stage of the broadband stream (off unless this is called): behind the synthesis, and in front of the copy back, the
 * device filters the samples it emits through the responses to validation microphones and reduces the pressures to energies per
 * hop and microphone; definitions, pressure sets, group order and arguments as for apv_stream_set_evaluation, with the stream's own
 * ranks (1..number_of_eigenvectors, or the list of apv_bb_set_rank_list) in place of the handle's rank list.  Called after
 * apv_bb_init, once, at any hop boundary: the histories start from silence and the totals from zero there.
 * apv_bb_process_block evaluates its hop in three launches (pressures; energies; totals and histories); apv_bb_process_signal with
 * cfg.out_layout = 1 evaluates a whole group of hops in the same three -- a group's samples are consecutive in time, and the
 * pressure kernel's bits do not depend on the launch -- and hop by hop with the channel-major layout.  The order in which a hop's
 * energy is summed depends on the hop size alone (csrc/kernels_bbeval.hip), so both paths give the same bits for the same samples.
 * States only such a stream has (apv_bb_get_state / apv_bb_set_state, counts in doubles):
 *   "eval_pressure" [Z][2 E + 1][H][Mv], the last hop's; read-only
 *   "eval_hops"     [n][Z][3 E + 1][Mv], the n hops of the last apv_bb_process_* call (the caller knows n); read-only
 *   "eval_totals"   [Z][3 E + 1][Mv], total = total + hop, one addition per hop in hop order
 *   "eval_history"  [Z][E + 1][Pv - 1][L], the newest Pv - 1 emitted samples of every evaluated group, oldest first
 * APV_ERR_ARG (nothing changed) without apv_bb_init, on a second call, for null pointers, Pv < 1, Mv < 1, Pv > 20465, n_ranks
 * outside 1..the stream's ranks, ranks not strictly ascending or not among the stream's.
 *                                                         replaces: Matlab/main.m:64-76, 120-130 with predictPressure.m:12-16 */
int  apv_bb_set_evaluation(apv_handle* h, int32_t Pv, int32_t Mv, const double* h_rvA, const double* h_rvB, int32_t n_ranks,
                           const int32_t* ranks);
/* "eval_totals" and both history buffers to zero: the next hop's totals equal its own energies; with
 * apv_bb_set_evaluation_spectra also "eval_spectra" and "eval_ring", with apv_bb_set_evaluation_detectability "eval_detect".
 * APV_ERR_ARG without such a stream. */
int  apv_bb_reset_evaluation(apv_handle* h);
/* Per-bin spectra of the broadband stream's evaluation stage (off unless called with on = 1): the definition of
 * apv_stream_set_evaluation_spectra -- frames of N = block_size pressure samples, H = hop_size apart, under the stream's sine
 * window, unnormalised rfft, |P|^2 added per bin, one addition per element and hop in hop order, float64, no atomics -- with hop t
 * counted from this call, a set "eval_ring" or apv_bb_reset_evaluation.  Behind the three launches of the evaluation stage three
 * more per launch of n hops (csrc/kernels_bbevalspec.hip): per pressure set and microphone a line of the newest N - H samples from
 * before and the launch's n H pressures; the stream's own windowed transform of its n frames; |P|^2 of the n hops added in hop order
 * by one owner per element.  The bits of the totals depend on the data and the hop order alone, so apv_bb_process_block and a group
 * of apv_bb_process_signal agree bit for bit.  The transforms' scratch has a budget of 64 MB (one hop where a hop is larger): a
 * group whose spectra exceed it runs as consecutive sub-launches of as many hops as fit.  States only such a stream has:
 *   "eval_spectra"  [Z][3 E + 1][K][Mv], K = N/2 + 1: per program [bright of the E ranks][dark ...][error ...][target]
 *   "eval_ring"     [Z (2 E + 1)][Mv][N]: the last N pressure samples per set (the order of "eval_pressure") and microphone,
 *                   oldest first
 * both readable and settable.  Called after apv_bb_set_evaluation, once, at any hop boundary: ring and spectra start from zero
 * there.  APV_ERR_ARG (nothing changed) without apv_bb_init, without apv_bb_set_evaluation, on a second call, for a value other
 * than 1, and for block_size > 4096 or any other size the float64 transforms refuse.
 *                                                         replaces: nothing in the reference (pwelch on the host) */
int  apv_bb_set_evaluation_spectra(apv_handle* h, int32_t on);
/* Perceptual detectability of the broadband stream's evaluated pressures: the definition of
 * apv_stream_set_evaluation_detectability -- error and leak per hop, program, evaluated rank and validation microphone from the
 * hop's spectra, f = 2 / N^2, the masker including bin 0, the sums over the bins 1.., the threshold in quiet as the leak's masker
 * with one program, float64, no atomics -- behind the transforms of every (sub-)launch of the spectra stage, on their scratch,
 * as three launches over all its hops (csrc/kernels_evaldetect.hip, the hop-batched forms).  The bits of a hop's values and of the
 * totals depend on the sizes, the data and the hop order alone, so apv_bb_process_block and a group of apv_bb_process_signal agree
 * bit for bit.  States only such a stream has:
 *   "eval_detect"       [Z][6 E][Mv]: per program [sum | max | number of hops with D > 1] of the error of the E ranks, then the
 *                       same three of the leak, since this call or the last reset (total = total + hop per hop); settable
 *   "eval_detect_hops"  [n][Z][2 E][Mv], the n hops of the last apv_bb_process_* call since this one (the caller knows n): per
 *                       program the error of the E ranks, then the leak; read-only
 * apv_bb_reset_evaluation zeroes "eval_detect".  h_G2 [N/2 + 1][n_channels], Cs, Ca, Leff: the tables of the model
 * (perceptual.PerceptualTables).  Called after apv_bb_set_evaluation_spectra, once, at any hop boundary: the totals start from zero
 * there; ring, spectra and everything else go on untouched.  APV_ERR_ARG (nothing changed) without apv_bb_init, without
 * apv_bb_set_evaluation_spectra, on a second call, for n_channels outside 1..512, a null table, a non-finite table entry or
 * constant, Ca <= 0, or N/2 + 1 + n_channels > 8192.     replaces: Matlab/ControlMethods/perceptualModel.m:192-206, on the device */
int  apv_bb_set_evaluation_detectability(apv_handle* h, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff);

/* ---- evaluation and the static solver, float64 ------------------------- */
/* p[t][m] = sum_s filter(rir[:, s, m], 1, x[:, s])[t].  h_x [T][L], h_rir [P][L][M], h_out [T][M].
 *                                                         replaces Matlab/ControlMethods/predictPressure.m:1-17 */
int  apv_predict_pressure(apv_handle* h, int32_t T, int32_t L, int32_t M, int32_t P, const double* h_x,
                          const double* h_rir, double* h_out);
/* Static (signal-independent) VAST filters from the impulse responses: h_gB [Nb][P][L], h_gD [Nd][P][L]
 * (vast.m's (mics, rirLength, sources) layout), h_w [J*L] (speaker-major taps).
 *                                                         replaces Matlab/ControlMethods/vast.m:1-97 */
int  apv_vast_static(apv_handle* h, int32_t Nb, int32_t Nd, int32_t P, int32_t L, int32_t J, int32_t modeling_delay,
                     int32_t reference_index, int32_t V, double mu, const double* h_gB, const double* h_gD, double* h_w);
/* The broadband Hankel statistics alone, as a hop and apv_vast_static launch them (kernel-level entry for tests):
 * R_j = sum_m Y_m Y_m^T for njobs (1..4) sets of rings and, with h_tstats, r = sum_m Y_m d_m for job 0, where
 * Y_m[(s, i)][c] = g_{s,m}[J - 1 - i + c], c < ncols, g = the ring unwrapped from `off` (sample J dropped when skip = 1) and
 * d_m[c] = the unwrapped target ring's sample toff + c.  h_stats [njobs][M*L][S] (row m*L + s), h_tstats [M][S] or NULL,
 * h_R [njobs][n][n], n = J L, h_r [n] or NULL (written only with h_tstats), all float64 on the host; *form_taken (may be NULL)
 * receives the form that ran.  No dialect scaling.  form: APV_HANKEL_AUTO is the launcher's own choice -- the displacement
 * form (one full sum per lag, then a walk down each diagonal) where 2 J - 1 <= 1024, its LDS (2 M (S + 8) doubles and the
 * work arrays) stays within 158 KiB and ncols + J + 2 <= S + 8, else the dense products on the matrix cores;
 * APV_HANKEL_DISPLACEMENT / APV_HANKEL_DENSE force one.  APV_ERR_ARG (nothing launched) unless 1 <= J, 1 <= L, 1 <= M,
 * n <= 4096, 0 <= off < S, skip in {0, 1}, ncols >= 1, ncols + J - 1 + skip <= S, 0 <= toff, toff + ncols <= S, and for
 * APV_HANKEL_DISPLACEMENT where that form does not fit.          replaces apvast.py:329-364 / apVast.m:410-447 (unscaled) */
#define APV_HANKEL_AUTO         0
#define APV_HANKEL_DISPLACEMENT 1
#define APV_HANKEL_DENSE        2
int  apv_hankel_statistics(apv_handle* h, int32_t J, int32_t L, int32_t M, int32_t S, int32_t off, int32_t skip, int32_t ncols,
                           int32_t toff, int32_t njobs, const double* h_stats, const double* h_tstats, int32_t form,
                           double* h_R, double* h_r, int32_t* form_taken);

/* ---- multi-GPU: bins sharded across ranks, one RCCL all-gather ---------- */
int  apv_comm_unique_id(char id_out[128]);                                /* rank 0 calls, then broadcasts */
int  apv_comm_init(apv_handle* h, const char id[128], int32_t rank, int32_t world);
/* gathers every rank's w shard [K][nV][L] into d_w_all [world*K][nV][L] (device) over xGMI.  Asynchronous:
 * it waits for the kernels already queued on the handle's stream, then runs on a second stream so that the
 * next apv_update_dev (into a different shard buffer) overlaps it; an update into the SAME shard buffer waits
 * for the gather.  apv_sync() waits for both streams. */
int  apv_allgather_filters_dev(apv_handle* h, const void* d_w_shard, void* d_w_all);
/* What the communicator itself reports (ncclCommCount / ncclCommUserRank); apv_comm_init already fails when they differ from
 * what it was given.  user_rank may be NULL. */
int  apv_comm_count(apv_handle* h, int32_t* n_ranks, int32_t* user_rank);
/* device time of the latest all-gather (HIP events on the communication stream) and the bytes this rank sent */
int  apv_comm_last_gather(apv_handle* h, float* elapsed_ms, size_t* bytes_per_rank);
/* all ranks of the communicator meet here (one-word ncclAllReduce); also drains the handle's compute stream */
int  apv_comm_barrier(apv_handle* h);
/* Diagnostics (tools/probes/stage_stamps.py; never set in normal use): with a device buffer of [zones][K][16] uint64 registered,
 * the order-16 update runs its diagnostic instantiation, in which lane 0 of every bin's wave stores the shader clock (s_memtime)
 * at the stage boundaries; NULL switches it off again.  The stamps go to this buffer only; no result depends on them. */
int  apv_debug_set_stamps(apv_handle* h, void* d_stamps);
/* Diagnostics (the leak checks of tests/test_gpu_stream_lifecycle.py): what the stream states and the scratch of running calls of
 * this process hold now: {device buffers, page-locked blocks, events, streams}.  The handle's own workspaces are not counted. */
int  apv_debug_live_resources(int32_t counts[4]);
/* hipDeviceSynchronize on the handle's device, and what that device is */
int  apv_device_sync(apv_handle* h);
int  apv_device_info(apv_handle* h, char name_out[128], int32_t* n_cus, int32_t* clock_mhz);

#ifdef __cplusplus
}
#endif
#endif /* APVAST_HIP_H */
