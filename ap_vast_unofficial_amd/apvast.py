"""Drop-in host surface: class ``apvast`` and function ``jdiag`` with the reference's
signatures (reference Python/apvast.py:20, 39-56, 153), computing on the MI355X through
libapvast_hip.so.  No CPU fallback: constructing the class without the HIP library or
without a GPU raises.

What is the same as the reference
  * positional constructor signature (apvast.py:40-56) and its three RuntimeErrors with the
    same messages (apvast.py:86-90, 154-155); LinAlgError when a dark matrix is not positive
    definite (apvast.py:21, 24)
  * ``process_input_buffers(input_A, input_B) -> (A, B, A_t, B_t)``: four lists of
    ``number_of_eigenvectors`` arrays of shape (hop_size, number_of_srcs), one per rank 1..V
    (apvast.py:406-422, 498-506); ``None`` for a zone that does not run (apvast.py:433-443)
  * ``rirs.mat`` ingest: ``rirA``/``rirB`` of shape (rir_len, L, M) (make_python_test.m:4, 18)
  * readable attributes: hop_size, window, number_of_srcs, number_of_mics, w_A/w_B, lambda_A/lambda_B, U_A/U_B,
    R_A_to_A/R_A_to_B/R_B_to_B/R_B_to_A, r_A/r_B, filter_spectra_A/B/A_t/B_t, input_spectrum_A/B (apvast.py:368-403);
    in subband mode they are per bin (leading axis K)
  * ``rir_A``, ``rir_B``, ``target_rir_A``, ``target_rir_B`` and ``mu`` may be reassigned between two hops, in both modes, as the
    reference reads them on every hop (apvast.py:161, 167-193): the samples already in keep ringing out through the response
    they were filtered with (lfilter's zi), the next hop on goes through the new one.  Targets are readable, built once as
    apvast.py:100-112 builds them and not re-derived from new rir_*; reference_index_* and modeling_delay are read only at
    construction, as in the reference
What is different (keyword-only, after ``perceptual``)
  * ``mode="subband"`` (default): one (R_B, R_D) pair, one GEVD and one filter PER FREQUENCY BIN from the
    current block's control-point spectra -- the fast path -- or, with ``statistics_hops=T``, from the spectra of the
    last T hops: R_B[k] = sum_t X_B^(h-t)[k]^H X_B^(h-t)[k], likewise R_D and r, the per-bin form of the reference's
    statistics buffer of several blocks (apvast.py:329-364).  ``statistics_hops="auto"`` takes T from
    ``statistics_buffer_length``: the whole blocks that many samples span, max(1, 1 + (S - N) // hop_size); the default 1
    keeps the single-block update (``statistics_buffer_length`` is used by ``"auto"`` only; ``filter_length`` is used by
    ``constrain_filter_length=True`` only, see below).  With T > 1 the attributes R_*, r_*, U_*, lambda_* are those of the window.
    ``statistics_forgetting=beta``, a float in (0, 1], is the recursive estimate instead: R_B[k] <- beta R_B[k] + X_B[k]^H X_B[k]
    per hop, likewise R_D and r, from zero before the first hop (1.0 accumulates every hop); one smoothing constant, no hard
    edge when a hop leaves, and memory that does not grow with the averaging time.  Fixed at construction; ``None`` (default)
    is off; it excludes ``statistics_hops > 1``, and R_*, r_*, U_*, lambda_* are then the running sums'.  ``dtype="f64"`` (default) runs every stage in
    float64 like the reference's lfilter / rfft / irfft (apvast.py:171-192, 202-203, 461-496); ``"f32"`` runs every
    stage in float32; ``"mixed"`` keeps the float32 FIR / STFT / overlap-add around a float64 joint diagonalisation.
    Up to 128 loudspeakers: above 64 the per-bin joint diagonalisation runs in float64 whatever ``dtype`` is
    (csrc/kernels_gevd128.hip), its filters and eigenvalues handed on in the dtype's format (complex64 / float32 for
    ``"f32"``); every rank 1..V, V <= number_of_srcs, is emitted.
  * ``constrain_filter_length=True`` (subband mode; default False): ``filter_length`` = J is honoured.  After the joint
    diagonalisation of a hop and before the output spectra, every filter -- zone programs that run, rank index v, loudspeaker l --
    is projected onto the spectra of causal J-tap responses: g = irfft(W[:, v, l], N) (numpy's convention: the imaginary parts of
    bins 0 and N/2 are discarded), g[J:] = 0, W'[:, v, l] = rfft(g, N), the constraint step of frequency-domain adaptive filters.
    W' is what the synthesis uses and what w_* / filter_spectra_* return; ``w_time_A`` / ``w_time_B`` return the taps g[:J] as
    float64 (V, J, L) -- the subband counterpart of the reference's J-tap w_A / w_B, loadable into a convolver -- and None before
    the first hop or for a zone that does not run.  Needs 1 <= filter_length <= block_size and modeling_delay < filter_length (the
    reference puts its target tap at J ref + delay); the target paths, a delta already, are untouched.  Combines with every dtype,
    statistics_hops, statistics_forgetting, perceptual, reassigned rir_* / mu, up to 128 loudspeakers and every block size.
    process_signal on such a stream runs its hops one after the other through the per-hop path (the same bits as the hop loop).
    Without the keyword the stream launches exactly what it launched before, and ``filter_length`` is stored and not used.
  * ``synthesis="fir"`` (with ``constrain_filter_length=True``; default ``"wola"``, the reference's weighted overlap-add): the J
    taps are applied to the inputs as time-domain FIR filters with no latency.  With x_z the input of zone program z (zero before
    the first hop), g_h the taps w_time_* return after hop h, g_-1 = 0, and for hop h, t = 0..H-1, n = h H + t, a = (t + 1) / H:
    y[z, v][n, l] = (1 - a) sum_j g_{h-1}[z, v, j, l] x_z[n - j] + a sum_j g_h[z, v, j, l] x_z[n - j], a linear cross-fade over
    the hop; the target outputs are the inputs delayed by modeling_delay in column reference_index_A.  Return shapes, w_*,
    lambda_*, w_time_* and everything else the design half leaves are unchanged; get_state() gains ``fir_synthesis_taps`` (zone
    programs that run, V, J, L) and ``fir_synthesis_history`` (2, J - 1), and ``out_overlap`` stays, untouched by the hops.
  * ``validation_rir_A`` / ``validation_rir_B`` (subband mode; both or neither, float64 (Pv, L, Mv), finite): an evaluation stage
    behind the synthesis of every hop.  The device filters the hop's own drive signals through the responses to validation
    microphones of both zones (Matlab/main.m:64-76 with predictPressure.m, carried across hops), keeps the pressures of the last
    hop, and accumulates per microphone the energies bright = sum p_own^2, dark = sum p_other^2, error = sum (p_target - p_own)^2
    and target = sum p_target^2, all in float64.  ``evaluation_ranks``: the ranks evaluated (None: every rank 1..V).
    ``evaluation_hops()``, ``evaluation_totals()``, ``predicted_pressure()`` fetch them when called, ``reset_evaluation()`` zeroes
    totals and histories, ``evaluation.metrics(totals)`` gives NMSE and contrast in dB (main.m:120-130); get_state() gains
    ``evaluation_history`` (Z, E + 1, Pv - 1, L) and ``evaluation_totals`` (Z, 3 E + 1, Mv).  Outputs, filters and every other state
    are those of the same stream without the keywords, bit for bit; process_signal runs such a stream hop by hop.
    In broadband mode the same stage is switched on by a method instead, ``ap.enable_evaluation(validation_rir_A,
    validation_rir_B, ranks=None)``, once and at any hop boundary; there process_signal evaluates a whole group of hops per launch.
  * ``evaluation_spectra=True`` (a bool; needs the validation responses): the evaluation stage also keeps the last block_size
    pressure samples per set and microphone and, after every hop t, transforms the frame that ends with the hop under the analysis
    window, P_t = rfft(window * p[(t + 1) H - N : (t + 1) H]) (zero before sample 0, unnormalised), and accumulates per bin
    bright += |P_own|^2, dark += |P_other|^2, error += |P_target - P_own|^2, target += |P_target|^2 in float64.
    ``evaluation_spectra()`` fetches them -- "bright", "dark", "error" (Z, E, Mv, K), "target" (Z, Mv, K) --
    ``evaluation.spectral_metrics`` gives contrast and NMSE per bin or band, ``reset_evaluation()`` zeroes them too, and
    get_state() gains ``evaluation_spectra`` (Z, 3 E + 1, K, Mv) and ``evaluation_ring`` (Z, 2 E + 1, Mv, N).  Everything else the
    stream computes is unchanged, bit for bit.  Block sizes up to 4096.
    In broadband mode the spectra are switched on by a method instead, ``ap.enable_evaluation_spectra()``, after
    ``enable_evaluation()``, once and at any hop boundary; there process_signal transforms a whole group of hops per launch.
  * ``evaluation_detectability=True`` (a bool; needs ``evaluation_spectra=True``): behind the spectra of every hop the device
    evaluates the second half of the masking model, evaluateDetectability (perceptualModel.m:192-206): with w2_S the squared
    weighting curve of a masker spectrum S (perceptualModel.m:118-139, un-normalised) and f = 2 / N^2, per program z, evaluated
    rank e and validation microphone m, error = sum_{k>=1} w2_{T[z,m]}[k] f |T - B|^2 -- the reproduction error masked by the
    program the listener wants -- and leak = sum_{k>=1} w2_{T[1-z,m]}[k] f |Dk|^2 -- the other program's leakage masked by this
    zone's own target (with one program: by silence, the threshold in quiet).  D = 1 is just audible.  float64 whatever dtype is;
    works with perceptual=False too (the tables are built once and shared).  ``evaluation_detectability()`` returns sums, maxima
    and audible-hop counts, ``evaluation_detectability_hops()`` the last call's hops, ``evaluation.detectability_metrics`` means
    and audible shares; get_state() gains ``evaluation_detectability`` (Z, 6 E + 1, Mv): the device's totals and, in a last row,
    the hops they cover.  Everything else the stream computes is unchanged, bit for bit.
    In broadband mode the detectability is switched on by a method instead, ``ap.enable_evaluation_detectability()``, after
    ``enable_evaluation_spectra()``, once and at any hop boundary; the totals and the hop count start there, and process_signal
    evaluates a whole group of hops in three launches whose bits are those of the hop loop.
  * ``effort_limit_db`` (subband mode; a float, (K,) or (2, K) array of dB values, row 0 = zone program A, ``+inf`` = no limit in
    that bin): the array effort e = sum_l |W[k, v, l]|^2 of every filter of a hop -- relative to the reference loudspeaker alone,
    whose effort is 0 dB -- is held to E = 10^(dB / 10) between the joint diagonalisation and the filter-length projection.  A
    filter with e <= E stays as it is; one above takes the filter of the largest lower rank that holds the limit, or is scaled by
    sqrt(E / e) when there is none.  ``effort_A`` / ``_B`` (K, V) return the efforts before the stage (linear), ``effort_rank_*``
    (K,) the rank the top filter was taken from (its own where it was scaled) and ``effort_gain_*`` (K,) its gain, all of the last
    hop; None without the keyword, before the first hop and for a zone that does not run.  The value can be reassigned between
    hops (not to None); w_*, w_time_* and the outputs are those of the limited filters, lambda_*, U_*, R_*, r_* and span_* are
    unchanged, and get_state() has the same keys.
  * ``validation_floor_db`` (subband mode; needs the validation responses; a float, (K,) or (2, K) array of dB values, row 0 =
    zone program A, ``-inf`` = no floor in that bin): the rank of every bin is chosen by the contrast the designed filters reach
    at the VALIDATION microphones (main.m:129-130), not at the control points they were fitted to.  With the static transfer
    functions G_z[k, m, l] = sum_j rv_z[j, l, m] exp(-2 pi i j k / N) (float64, once at construction) the stage predicts per bin k
    and filter v bright = sum_m |sum_l G_own[k, m, l] W[k, v, l]|^2 and dark likewise with the other zone's responses; a filter is
    admissible if bright >= 10^(dB / 10) dark.  Between the joint diagonalisation (span included) and the effort limit every
    filter takes the filter of the largest admissible rank at or below its own, or of the rank of largest contrast at or below
    its own when none is admissible.  ``validation_bright_A`` / ``_B``, ``validation_dark_*`` (K, V) return the energies before the
    choice, ``validation_source_*`` (K, V) int32 the index of the filter each filter was taken from (-1: left as it is) and
    ``validation_rank_*`` (K,) the rank of the top filter's source, all of the last hop; None without the keyword, before the
    first hop and for a zone that does not run.  The value can be reassigned between hops (not to None); w_*, filter_spectra_*,
    w_time_* and the outputs are those of the chosen filters, lambda_*, U_*, R_*, r_*, span_* are unchanged, and get_state() has
    the same keys.  ``evaluation.validation_contrast_db`` turns the energies into dB.
  * ``mode="broadband"``: the reference's own time-domain algorithm (one (J L) x (J L) pair per zone from
    ``statistics_buffer_length`` samples, apvast.py:329-422), float64 on the device, checked against the
    golden outputs of the reference (tests/test_gpu_broadband.py).
  * an assigned response must have the constructor's shape and be finite (ValueError otherwise, nothing changed); the class keeps
    a READ-ONLY float64 copy, so an in-place edit raises where the reference would see it.  Everything assigned since the last
    hop is applied at the start of the next one
  * outputs are fresh arrays (the reference returns views into its overlap buffers that the next
    call overwrites, apvast.py:500-504).
  * the per-hop attributes (w_*, lambda_*, input_spectrum_*, filter_spectra_*, U_*, R_*, r_*) are fetched from the device
    WHEN READ, not at the end of every hop: process_input_buffers moves nothing but the hop in and the drive signals out.
    A hop whose eigen-iteration stops at its sweep cap still returns its outputs and warns (ConvergenceWarning;
    ``not_converged`` counts such hops); a dark matrix that is not positive definite raises LinAlgError as in the reference.
  * ``perceptual=True``: the reference's Python class calls the third-party
    ``libdetectability`` (apvast.py:4, 77-83), which it does not vendor; here the weighting is the van de Par
    masking model carried by the reference's MATLAB twin (perceptualModel.m), evaluated per block on the
    device.  Parity for it is unpinned (no MATLAB here).
"""
import collections

import numpy as np

from . import _capi
from ._capi import ConvergenceWarning  # noqa: F401  (re-exported: what a capped eigen-iteration warns with)

EXPERIMENTAL_NORMALIZE_GAINS = True     # apvast.py:6 (only used by the perceptual model)
EXPERIMENTAL_REGULARIZATION = True      # apvast.py:7: True -> B + 1e-7 I, False -> B + 1e-8 ||B||_2 I


def load_rirs(path):
    """scipy.io.loadmat ingest of the reference's rirs.mat (make_python_test.m:4): (rirA, rirB)."""
    import scipy.io
    mat = scipy.io.loadmat(path)
    return np.ascontiguousarray(mat["rirA"], dtype=np.float64), np.ascontiguousarray(mat["rirB"], dtype=np.float64)


_jdiag_engine = None


def jdiag(A, B, device=0):
    """Joint diagonalisation on the GPU: (U, D) with U^H (B + reg I) U = I, U^H A U = D, D descending
    and returned as a diagonal MATRIX, as apvast.py:20-36 does.  Real symmetric pairs up to n = 4096, complex Hermitian
    pairs up to n = 1024 (beyond 64 through the real embedding of order 2n, csrc/kernels_jdiag_cplx.hip).
    Raises numpy.linalg.LinAlgError when the loaded B is not positive definite (apvast.py:21)."""
    global _jdiag_engine
    A = np.asarray(A)
    B = np.asarray(B)
    n = A.shape[0]
    if A.shape != (n, n) or B.shape != (n, n):
        raise ValueError("jdiag expects two square matrices of equal size")
    cplx = np.iscomplexobj(A) or np.iscomplexobj(B)
    if n > _capi.MAX_N and n > (1024 if cplx else 4096):
        raise NotImplementedError("GPU jdiag: complex Hermitian pairs up to n = 1024; real symmetric pairs up to n = 4096")
    mode = _capi.REG_ABS if EXPERIMENTAL_REGULARIZATION else _capi.REG_REL
    key = (device, mode)
    if _jdiag_engine is None or _jdiag_engine[0] != key:
        eng = _capi.Engine(1, 4, 4, reg_mode=mode, reg_dark=1e-7 if mode == _capi.REG_ABS else 1e-8, device=device)
        _jdiag_engine = (key, eng)
    if n > _capi.MAX_N:
        eng = _jdiag_engine[1]
        U, lam = eng.jdiag_large_complex(A[None], B[None]) if cplx else eng.jdiag_large(A[None], B[None])
        return U[0], np.diag(lam[0])
    U, lam = _jdiag_engine[1].jdiag_batched(A[None], B[None])
    U, lam = U[0], lam[0]
    if not cplx:
        U = np.ascontiguousarray(U.real)
    return U, np.diag(lam)


class apvast:
    def __init__(self,
                 block_size: int,
                 rir_A,
                 rir_B,
                 filter_length: int,
                 modeling_delay: int,
                 reference_index_A: int,
                 reference_index_B: int,
                 number_of_eigenvectors: int,
                 mu: float,
                 statistics_buffer_length: int,
                 hop_size: int = None,
                 sampling_rate: int = 48000,
                 run_A: bool = True,
                 run_B: bool = True,
                 perceptual: bool = True,
                 *,
                 mode: str = "subband",
                 dialect: str = "python",
                 device: int = 0,
                 dtype: str = "f64",
                 seed=None,
                 fullscale_db_spl: float = 94.0,
                 max_sweeps: int = 0,
                 sweep_tol2: float = 0.0,
                 constrain_filter_length=False,
                 synthesis="wola",
                 validation_rir_A=None,
                 validation_rir_B=None,
                 evaluation_ranks=None,
                 evaluation_spectra=False,
                 evaluation_detectability=False,
                 statistics_forgetting=None,
                 mu_profile=None,
                 rank_profile=None,
                 contrast_floor_db=None,
                 validation_floor_db=None,
                 effort_limit_db=None,
                 statistics_hops=1):
        self.block_size = block_size
        self.filter_length = filter_length
        self.modeling_delay = modeling_delay
        self.reference_index_A = reference_index_A
        self.reference_index_B = reference_index_B
        self.number_of_eigenvectors = number_of_eigenvectors
        self._mu = float(mu)
        self.sampling_rate = sampling_rate
        self.statistics_buffer_length = statistics_buffer_length
        self.run_A = run_A
        self.run_B = run_B
        self.perceptual = perceptual
        self.mode, self.dialect, self.dtype = mode, dialect, dtype

        if self.block_size % 2 != 0:
            raise RuntimeError("block size must be modulo 2")                 # apvast.py:86-87
        if rir_A.shape != rir_B.shape:
            raise RuntimeError("rirs of unequal size")                        # apvast.py:89-90
        self._fullscale_db_spl = fullscale_db_spl
        self._max_sweeps = int(max_sweeps)       # Jacobi sweep cap (0 = default); a hop that reaches it still returns its outputs and warns (ConvergenceWarning)
        if mode not in ("subband", "broadband"):
            raise ValueError("mode must be 'subband' or 'broadband'")
        if dialect not in ("python", "matlab"):
            raise ValueError("dialect must be 'python' or 'matlab'")
        if dtype not in ("f64", "f32", "mixed"):
            raise ValueError("dtype must be 'f64' (float64 end to end, the reference's arithmetic), 'f32' (float32 end to "
                             "end) or 'mixed' (float32 FIR/STFT/overlap-add around a float64 joint diagonalisation)")
        if not (run_A or run_B):
            raise ValueError("at least one of run_A / run_B must be True")

        self.hop_size = hop_size if hop_size else self.block_size // 2        # apvast.py:93
        self.statistics_hops = self._resolve_statistics_hops(statistics_hops, statistics_buffer_length, block_size,
                                                             self.hop_size, mode)
        self.statistics_forgetting = self._check_statistics_forgetting(statistics_forgetting, self.statistics_hops, mode)
        self.constrain_filter_length = self._check_constrain_filter_length(constrain_filter_length, filter_length, block_size,
                                                                           modeling_delay, mode)
        self.synthesis = self._check_synthesis(synthesis, self.constrain_filter_length, mode)
        self.window = np.sin(np.pi / self.block_size * np.arange(self.block_size)).reshape(-1, 1)   # apvast.py:94
        self.rir_length, self.number_of_srcs, self.number_of_mics = rir_A.shape  # apvast.py:97-99
        L, M, N, H = self.number_of_srcs, self.number_of_mics, self.block_size, self.hop_size
        self._evaluation = self._check_evaluation(validation_rir_A, validation_rir_B, evaluation_ranks, L, number_of_eigenvectors, mode)
        self._evaluation_spectra = self._check_evaluation_spectra(evaluation_spectra, self._evaluation, mode)
        self._evaluation_detectability = self._check_evaluation_detectability(evaluation_detectability, self._evaluation_spectra, mode)
        # the per-bin span: which of its three parts exist is fixed here, their values may be reassigned between hops
        self._span = {"mu_profile": self._check_mu_profile(mu_profile, N // 2 + 1, mode),
                      "rank_profile": self._check_rank_profile(rank_profile, N // 2 + 1, L, mode),
                      "contrast_floor_db": self._check_contrast_floor_db(contrast_floor_db, mode)}
        self._span_pending = False
        # the per-bin array-effort limit: whether the stage exists is fixed here, its values may be reassigned between hops
        self._effort_limit_db = self._check_effort_limit_db(effort_limit_db, N // 2 + 1, mode)
        self._effort_pending = False
        # the rank choice at the validation microphones: whether the stage exists is fixed here, its floor may be reassigned
        self._validation_floor_db = self._check_validation_floor_db(validation_floor_db, N // 2 + 1, self._evaluation, mode)
        self._validation_pending = False
        self._init_responses(rir_A, rir_B)
        if mode == "broadband":
            self._init_broadband(device, seed)
            return
        V = int(number_of_eigenvectors)
        if not 1 <= V <= L:
            raise ValueError("subband mode: number_of_eigenvectors must be in 1..number_of_srcs")
        self._ranks = list(range(1, V + 1))            # the reference emits every rank 1..V (apvast.py:406-422)
        self._K = N // 2 + 1
        if dialect == "python":
            reg_mode = _capi.REG_ABS if EXPERIMENTAL_REGULARIZATION else _capi.REG_REL
            reg_dark = 1e-7 if EXPERIMENTAL_REGULARIZATION else 1e-8          # apvast.py:22-27
            reg_bright = 0.0
        else:
            reg_mode, reg_dark, reg_bright = _capi.REG_REL, 5e-3, 1e-8        # apVast.m:552-569
        zones = (1 if run_A else 0) | (2 if run_B else 0)
        tables = None
        if self._evaluation_detectability:
            # the detectability stage takes the model's tables before the stream is initialised; the design weighting below
            # reuses them
            from .perceptual import PerceptualTables
            tables = PerceptualTables(N, sampling_rate, fullscale_db_spl)
        self.detectability_model = tables               # what the device received; None without the keyword
        self._eng = _capi.Engine(self._K, L, M, ranks=self._ranks, mu=self._mu, compute_dtype="f32" if dtype == "f32" else "f64",
                                 reg_mode=reg_mode, reg_dark=reg_dark, reg_bright=reg_bright, device=device,
                                 block_size=N, hop_size=H, n_zones=zones, frontend="f32" if dtype == "mixed" else None,
                                 max_sweeps=self._max_sweeps, sweep_tol2=sweep_tol2,
                                 out_layout=1,     # the device emits (hop, loudspeaker) arrays: nothing to transpose here
                                 stat_hops=self.statistics_hops, stat_forgetting=self.statistics_forgetting,
                                 filter_taps=int(filter_length) if self.constrain_filter_length else 0,
                                 synthesis=self.synthesis, evaluation=self._evaluation,
                                 evaluation_spectra=self._evaluation_spectra, span=self._span_args(),
                                 effort_limit=self._effort_table(),
                                 validation_span=self._validation_span_args(),
                                 evaluation_detectability=tables if self._evaluation_detectability else None)
        self._eng.stream_init(rir_A, rir_B, reference_index_A, reference_index_B, modeling_delay)
        if perceptual:
            # the masking model carried by the MATLAB twin (perceptualModel.m); per-block curves are formed on the
            # device from the target spectra, normalised as the dialect prescribes (apvast.py:322-324 /
            # perceptualModel.m:177-190)
            from .perceptual import PerceptualTables
            self.model = tables if tables is not None else PerceptualTables(N, sampling_rate, fullscale_db_spl)
            self._eng.stream_set_perceptual(self.model, dialect)
        self._n_out = (int(run_A) + int(run_B)) * V * L + 2 * L
        tgt = np.zeros((N, L))
        tgt[modeling_delay, reference_index_A] = 1.0                           # apvast.py:389-390: one filter for A_t and B_t
        tspec = np.fft.rfft(tgt, axis=0)
        self.filter_spectra_A_t = [tspec.copy() for _ in range(V)]             # apvast.py:418, 422
        self.filter_spectra_B_t = [tspec.copy() for _ in range(V)]
        if dialect == "python":
            # apvast.py:124-129: response buffers start as 1e-3 * randn, drawn from the global NumPy RNG in this
            # order; pass seed=... for a private, reproducible generator instead
            rs = np.random if seed is None else np.random.RandomState(seed)
            resp = [1e-3 * rs.randn(N, L, M) for _ in range(4)]               # A->A, A->B, B->A, B->B
            tresp = [1e-3 * rs.randn(N, M) for _ in range(2)]
            self.set_state({"response": np.stack(resp), "target_response": np.stack(tresp)})
        self._hops = 0                      # attributes of apvast.py:368-403 exist once a hop has run
        self._detect_hops = 0               # hops since construction, reset_evaluation() or a restored evaluation_detectability
        self._sb_cache = {}

    @staticmethod
    def _resolve_statistics_hops(value, statistics_buffer_length, block_size, hop_size, mode):
        """statistics_hops as an int in 1.._capi.MAX_STAT_HOPS.  "auto": the whole blocks that statistics_buffer_length samples
        span, max(1, 1 + (S - N) // H) (the reference's example: S = 512, N = 256, H = 128 -> 3), capped at the largest window.
        Broadband mode has its own statistics buffer: only 1 and "auto" (which mean nothing there) are accepted."""
        if isinstance(value, str):
            if value != "auto":
                raise ValueError("statistics_hops must be an int in 1..%d or 'auto'" % _capi.MAX_STAT_HOPS)
            if mode == "broadband":
                return 1
            T = max(1, 1 + (int(statistics_buffer_length) - int(block_size)) // int(hop_size))
            return min(T, _capi.MAX_STAT_HOPS)
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= _capi.MAX_STAT_HOPS:
            raise ValueError("statistics_hops must be an int in 1..%d or 'auto'" % _capi.MAX_STAT_HOPS)
        if mode == "broadband" and int(value) > 1:
            raise ValueError("statistics_hops > 1 is a subband keyword: broadband mode averages over statistics_buffer_length samples")
        return int(value)

    @staticmethod
    def _check_statistics_forgetting(value, statistics_hops, mode):
        """statistics_forgetting as None (off) or a float in (0, 1]."""
        if value is None:
            return None
        if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not 0.0 < float(value) <= 1.0:
            raise ValueError("statistics_forgetting must be None or a number in (0, 1]")       # (NaN fails the comparison)
        if mode == "broadband":
            raise ValueError("statistics_forgetting is a subband keyword: broadband mode averages over statistics_buffer_length samples")
        if statistics_hops > 1:
            raise ValueError("statistics_forgetting and statistics_hops > 1 exclude each other: one estimator per stream")
        return float(value)

    @staticmethod
    def _check_constrain_filter_length(value, filter_length, block_size, modeling_delay, mode):
        """constrain_filter_length as a bool; True needs subband mode, 1 <= filter_length <= block_size and
        modeling_delay < filter_length."""
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError("constrain_filter_length must be a bool")
        if not value:
            return False
        if mode == "broadband":
            raise ValueError("constrain_filter_length is a subband keyword: broadband mode designs filter_length-tap filters by construction")
        if isinstance(filter_length, bool) or not isinstance(filter_length, (int, np.integer)) or not 1 <= int(filter_length) <= int(block_size):
            raise ValueError("constrain_filter_length: filter_length must be an int in 1..block_size")
        if not int(modeling_delay) < int(filter_length):
            raise ValueError("constrain_filter_length: modeling_delay must be below filter_length (the target tap has to lie inside "
                             "the filter)")
        return True

    @staticmethod
    def _check_synthesis(value, constrain_filter_length, mode):
        """synthesis as "wola" or "fir"; "fir" needs subband mode and constrain_filter_length=True (it applies the J taps)."""
        if not isinstance(value, str) or value not in ("wola", "fir"):
            raise ValueError("synthesis must be 'wola' (weighted overlap-add, the reference's) or 'fir' (the constrained filters "
                             "as time-domain FIR filters)")
        if value == "wola":
            return value
        if mode == "broadband":
            raise ValueError("synthesis='fir' is a subband keyword: broadband mode has its own time-domain filters")
        if not constrain_filter_length:
            raise ValueError("synthesis='fir' needs constrain_filter_length=True: it applies the filter_length taps of w_time_*")
        return value

    @staticmethod
    def _check_evaluation(rv_A, rv_B, ranks, L, V, mode):
        """The evaluation keywords as None (off) or (rv_A, rv_B, ranks): float64 (Pv, L, Mv) responses of equal shape, finite,
        and the evaluated ranks, strictly ascending within 1..V (None: every rank)."""
        if rv_A is None and rv_B is None:
            if ranks is not None:
                raise ValueError("evaluation_ranks needs validation_rir_A and validation_rir_B")
            return None
        if mode == "broadband":
            raise ValueError("validation_rir_A / validation_rir_B are a subband keyword: broadband mode has no evaluation stage")
        a, b = apvast._check_validation_rirs(rv_A, rv_B, L)
        r = apvast._check_rank_subset(ranks, range(1, int(V) + 1), "evaluation_ranks must be None or a strictly ascending list of ranks "
                                      "within 1..number_of_eigenvectors")
        return a, b, r

    @staticmethod
    def _check_validation_rirs(rv_A, rv_B, L):
        """Float64 copies of the responses to the validation microphones: both given, one shape (Pv, L, Mv), finite."""
        if rv_A is None or rv_B is None:
            raise ValueError("validation_rir_A and validation_rir_B go together: both or neither")
        a, b = np.array(rv_A, dtype=np.float64), np.array(rv_B, dtype=np.float64)
        if a.ndim != 3 or a.shape != b.shape:
            raise ValueError(f"validation_rir_A and validation_rir_B must have one shape (Pv, L, Mv), got {a.shape} and {b.shape}")
        if a.shape[1] != L or a.shape[0] < 1 or a.shape[2] < 1:
            raise ValueError(f"validation_rir_*: (Pv, L, Mv) with L = {L} loudspeakers (the constructor's) and Pv, Mv >= 1, got {a.shape}")
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            raise ValueError("validation_rir_A and validation_rir_B must be finite")
        return a, b

    @staticmethod
    def _check_rank_subset(ranks, emitted, message):
        """The evaluated ranks as a list of ints: None -> every emitted rank, else a strictly ascending, non-empty subset of them."""
        emitted = [int(v) for v in emitted]
        if ranks is None:
            return emitted
        try:
            r = list(ranks)
        except TypeError:
            raise ValueError(message)
        ok = len(r) >= 1 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and int(v) in emitted for v in r)
        if not ok or any(int(r[i]) <= int(r[i - 1]) for i in range(1, len(r))):
            raise ValueError(message)
        return [int(v) for v in r]

    @staticmethod
    def _check_evaluation_spectra(value, evaluation, mode):
        """evaluation_spectra as a bool; True needs subband mode and the evaluation stage."""
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError("evaluation_spectra must be a bool")
        if not value:
            return False
        if mode == "broadband":
            raise ValueError("evaluation_spectra is a subband keyword: broadband mode has no evaluation stage")
        if evaluation is None:
            raise ValueError("evaluation_spectra needs validation_rir_A and validation_rir_B")
        return True

    @staticmethod
    def _check_evaluation_detectability(value, evaluation_spectra, mode):
        """evaluation_detectability as a bool; True needs subband mode and the per-bin spectra."""
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError("evaluation_detectability must be a bool")
        if not value:
            return False
        if mode == "broadband":
            raise ValueError("evaluation_detectability is a subband keyword: broadband mode has no evaluation stage")
        if not evaluation_spectra:
            raise ValueError("evaluation_detectability needs evaluation_spectra=True")
        return True

    # ---- the per-bin span (mu_profile, rank_profile, contrast_floor_db) -------------------------------------
    @staticmethod
    def _span_table(name, value, K, check):
        a = np.asarray(value)
        if a.shape == (K,):
            a = np.stack([a, a])
        if a.shape != (2, K):
            raise ValueError(f"{name} must have shape ({K},) (both zone programs) or (2, {K}) (one row per program), got {a.shape}")
        a = check(a)
        a.flags.writeable = False
        return a

    @staticmethod
    def _check_mu_profile(value, K, mode):
        """mu_profile as a read-only (2, K) float64 array, or None: finite, non-negative factors of mu per bin."""
        if value is None:
            return None
        if mode == "broadband":
            raise ValueError("mu_profile is a subband keyword: broadband mode designs one filter for the whole band")

        def check(a):
            if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
                raise ValueError("mu_profile must hold finite, non-negative floats")
            a = np.array(a, dtype=np.float64)
            if not np.isfinite(a).all() or (a < 0).any():
                raise ValueError("mu_profile must hold finite, non-negative floats")
            return a
        return apvast._span_table("mu_profile", value, K, check)

    @staticmethod
    def _check_rank_profile(value, K, L, mode):
        """rank_profile as a read-only (2, K) int32 array, or None: the largest rank of each bin, integers in 1..L."""
        if value is None:
            return None
        if mode == "broadband":
            raise ValueError("rank_profile is a subband keyword: broadband mode designs one filter for the whole band")

        def check(a):
            if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"rank_profile must hold integers in 1..{L} (number_of_srcs)")
            if (a < 1).any() or (a > L).any():
                raise ValueError(f"rank_profile must hold integers in 1..{L} (number_of_srcs)")
            return np.array(a, dtype=np.int32)
        return apvast._span_table("rank_profile", value, K, check)

    @staticmethod
    def _check_contrast_floor_db(value, mode):
        """contrast_floor_db as a finite float, or None."""
        if value is None:
            return None
        if mode == "broadband":
            raise ValueError("contrast_floor_db is a subband keyword: broadband mode designs one filter for the whole band")
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)) or not np.isfinite(value):
            raise ValueError("contrast_floor_db must be a finite float")
        _capi.contrast_floor(value)          # ... whose 10^(dB / 10) is a positive, finite double
        return float(value)

    def _span_args(self):
        """The span as _capi.Engine takes it; None when no part was given."""
        s = self._span
        if all(v is None for v in s.values()):
            return None
        return {"mu_profile": s["mu_profile"], "rank_cap": s["rank_profile"], "contrast_floor_db": s["contrast_floor_db"]}

    def _set_span_part(self, name, value):
        span = self.__dict__.get("_span")
        if span is None or span[name] is None:
            raise ValueError(f"{name} was not given at construction: the parts of the span are fixed there")
        K, L = self._K, self.number_of_srcs
        new = {"mu_profile": lambda: self._check_mu_profile(value, K, self.mode),
               "rank_profile": lambda: self._check_rank_profile(value, K, L, self.mode),
               "contrast_floor_db": lambda: self._check_contrast_floor_db(value, self.mode)}[name]()
        if new is None:
            raise ValueError(f"{name} cannot be removed: the parts of the span are fixed at construction")
        span[name] = new
        self._span_pending = True

    # an assignment between two hops takes effect at the next one (_apply_live); `mu` stays the common factor of mu_profile
    mu_profile = property(lambda self: self._span["mu_profile"], lambda self, v: self._set_span_part("mu_profile", v))
    rank_profile = property(lambda self: self._span["rank_profile"], lambda self, v: self._set_span_part("rank_profile", v))
    contrast_floor_db = property(lambda self: self._span["contrast_floor_db"],
                                 lambda self, v: self._set_span_part("contrast_floor_db", v))

    def _span_output(self, zone, what):
        """span_rank (K,) int32 / span_contrast (K, L) float64 of the last hop, fetched when read.  None for an object without a
        span, before the first hop, for a zone program that does not run, and for the contrast without a floor."""
        if self.mode == "broadband" or self._span_args() is None or self._hops == 0 or not (self.run_A, self.run_B)[zone]:
            return None
        return self._eng.span(zone)[what]

    span_rank_A = property(lambda self: self._span_output(0, 0))
    span_rank_B = property(lambda self: self._span_output(1, 0))
    span_contrast_A = property(lambda self: self._span_output(0, 1))
    span_contrast_B = property(lambda self: self._span_output(1, 1))

    # ---- the per-bin array-effort limit (effort_limit_db) ---------------------------------------------------
    @staticmethod
    def _check_effort_limit_db(value, K, mode):
        """effort_limit_db as a read-only (2, K) float64 array of dB values, or None: a float, (K,) or (2, K); +inf = no limit."""
        if value is None:
            return None
        if mode == "broadband":
            raise ValueError("effort_limit_db is a subband keyword: broadband mode designs one filter for the whole band")
        bad = "effort_limit_db must hold dB values that are floats, not NaN and not -inf (+inf: no limit in that bin)"
        if isinstance(value, (bool, np.bool_, str, bytes)):
            raise ValueError(bad)
        try:
            a = np.asarray(value)
        except Exception:
            raise ValueError(bad) from None
        if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(bad)
        a = np.array(a, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((2, K), float(a))
        elif a.shape == (K,):
            a = np.stack([a, a])
        if a.shape != (2, K):
            raise ValueError(f"effort_limit_db must be a float or have shape ({K},) (both zone programs) or (2, {K}) (one row per "
                             f"program), got {a.shape}")
        if np.isnan(a).any() or np.isneginf(a).any():
            raise ValueError(bad)
        with np.errstate(over="ignore"):
            lin = 10.0 ** (a / 10.0)
        if (lin <= 0).any():
            raise ValueError("effort_limit_db: 10^(dB / 10) must be a positive double")
        a.flags.writeable = False
        return a

    def _effort_table(self):
        """The limit as _capi.Engine takes it, (2, K) linear; None without the keyword."""
        if self._effort_limit_db is None:
            return None
        with np.errstate(over="ignore"):
            return 10.0 ** (self._effort_limit_db / 10.0)

    def _set_effort_limit_db(self, value):
        if self.__dict__.get("_effort_limit_db") is None:
            raise ValueError("effort_limit_db was not given at construction: whether the stage exists is fixed there")
        new = self._check_effort_limit_db(value, self._K, self.mode)
        if new is None:
            raise ValueError("effort_limit_db cannot be removed: whether the stage exists is fixed at construction (+inf lifts the limit)")
        self._effort_limit_db = new
        self._effort_pending = True

    # an assignment between two hops takes effect at the next one (_apply_live)
    effort_limit_db = property(lambda self: self._effort_limit_db, _set_effort_limit_db)

    def _effort_output(self, zone, what):
        """effort (K, V) float64 linear / effort_rank (K,) int32 / effort_gain (K,) float64 of the last hop, fetched when read.  None
        for an object without the keyword, before the first hop and for a zone program that does not run."""
        if self.mode == "broadband" or self._effort_limit_db is None or self._hops == 0 or not (self.run_A, self.run_B)[zone]:
            return None
        return self._eng.effort(zone)[what]

    effort_A = property(lambda self: self._effort_output(0, 0))
    effort_B = property(lambda self: self._effort_output(1, 0))
    effort_rank_A = property(lambda self: self._effort_output(0, 1))
    effort_rank_B = property(lambda self: self._effort_output(1, 1))
    effort_gain_A = property(lambda self: self._effort_output(0, 2))
    effort_gain_B = property(lambda self: self._effort_output(1, 2))

    # ---- the rank choice at the validation microphones (validation_floor_db) --------------------------------
    @staticmethod
    def _check_validation_floor_db(value, K, evaluation, mode):
        """validation_floor_db as a read-only (2, K) float64 array of dB values, or None: a float, (K,) or (2, K); -inf = no floor."""
        if value is None:
            return None
        if mode == "broadband":
            raise ValueError("validation_floor_db is a subband keyword: broadband mode has no evaluation stage")
        if evaluation is None:
            raise ValueError("validation_floor_db needs validation_rir_A and validation_rir_B")
        bad = "validation_floor_db must hold dB values that are floats, not NaN and not +inf (-inf: no floor in that bin)"
        if isinstance(value, (bool, np.bool_, str, bytes)):
            raise ValueError(bad)
        try:
            a = np.asarray(value)
        except Exception:
            raise ValueError(bad) from None
        if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise ValueError(bad)
        a = np.array(a, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((2, K), float(a))
        elif a.shape == (K,):
            a = np.stack([a, a])
        if a.shape != (2, K):
            raise ValueError(f"validation_floor_db must be a float or have shape ({K},) (both zone programs) or (2, {K}) (one row "
                             f"per program), got {a.shape}")
        if np.isnan(a).any() or np.isposinf(a).any():
            raise ValueError(bad)
        with np.errstate(over="ignore"):
            lin = 10.0 ** (a / 10.0)
        if not np.isfinite(lin).all() or (lin[np.isfinite(a)] <= 0).any():
            raise ValueError("validation_floor_db: 10^(dB / 10) must be a positive, finite double (-inf: no floor)")
        a.flags.writeable = False
        return a

    @staticmethod
    def validation_transfer(rv, block_size):
        """G[k, m, l] = sum_j rv[j, l, m] exp(-2 pi i j k / N), k = 0 .. N/2: the response of (Pv, L, Mv) validation responses at
        the bin centres, (K, Mv, L) complex128, for any Pv (taps beyond N fold back onto the N bin frequencies)."""
        rv = np.asarray(rv, dtype=np.float64)
        N = int(block_size)
        Pv, L, Mv = rv.shape
        folded = np.zeros((N, L, Mv))
        for j0 in range(0, Pv, N):
            part = rv[j0:j0 + N]
            folded[:part.shape[0]] += part
        return np.ascontiguousarray(np.fft.rfft(folded, axis=0).transpose(0, 2, 1))

    def _validation_floor_table(self):
        """The floor as _capi.Engine takes it, (2, K) linear phi (0 = no floor)."""
        return 10.0 ** (self._validation_floor_db / 10.0)

    def _validation_span_args(self):
        """(floor, G_A, G_B) as _capi.Engine takes them; None without the keyword."""
        if self._validation_floor_db is None:
            return None
        rvA, rvB, _ = self._evaluation
        return (self._validation_floor_table(), self.validation_transfer(rvA, self.block_size),
                self.validation_transfer(rvB, self.block_size))

    def _set_validation_floor_db(self, value):
        if self.__dict__.get("_validation_floor_db") is None:
            raise ValueError("validation_floor_db was not given at construction: whether the stage exists is fixed there")
        new = self._check_validation_floor_db(value, self._K, self._evaluation, self.mode)
        if new is None:
            raise ValueError("validation_floor_db cannot be removed: whether the stage exists is fixed at construction (-inf lifts "
                             "the floor)")
        self._validation_floor_db = new
        self._validation_pending = True

    # an assignment between two hops takes effect at the next one (_apply_live)
    validation_floor_db = property(lambda self: self._validation_floor_db, _set_validation_floor_db)

    def _validation_output(self, zone, what):
        """validation_bright / _dark (K, V) float64, _source (K, V) int32, _rank (K,) int32 of the last hop, fetched when read.
        None for an object without the keyword, before the first hop and for a zone program that does not run."""
        if self.mode == "broadband" or self._validation_floor_db is None or self._hops == 0 or not (self.run_A, self.run_B)[zone]:
            return None
        return self._eng.validation_span(zone, what)

    validation_bright_A = property(lambda self: self._validation_output(0, 0))
    validation_bright_B = property(lambda self: self._validation_output(1, 0))
    validation_dark_A = property(lambda self: self._validation_output(0, 1))
    validation_dark_B = property(lambda self: self._validation_output(1, 1))
    validation_source_A = property(lambda self: self._validation_output(0, 2))
    validation_source_B = property(lambda self: self._validation_output(1, 2))
    validation_rank_A = property(lambda self: self._validation_output(0, 3))
    validation_rank_B = property(lambda self: self._validation_output(1, 3))

    # ---- the evaluation stage (validation_rir_A / validation_rir_B): read from the device when asked for ------------------
    def _eval_stage(self):
        """(rv_A, rv_B, ranks) of the object's evaluation stage -- the constructor's in subband mode, enable_evaluation()'s in
        broadband mode -- or None."""
        d = self.__dict__
        return d.get("_bb_evaluation") if d.get("mode") == "broadband" else d.get("_evaluation")

    def _eval_dims(self):
        if self._eval_stage() is None:
            raise RuntimeError("this object has no evaluation stage: pass validation_rir_A and validation_rir_B (subband mode) "
                               "or call enable_evaluation() (broadband mode)")
        a, _, r = self._eval_stage()
        return int(self.run_A) + int(self.run_B), len(r), a.shape[0], a.shape[2]

    def enable_evaluation(self, validation_rir_A, validation_rir_B, ranks=None):
        """Broadband mode: switch the evaluation stage on, once, at any hop boundary (before the first hop included).  From here
        on the device filters every hop it emits through the responses to the validation microphones -- float64 (Pv, L, Mv), finite,
        Pv <= 20465 -- and keeps pressures, energies per hop and totals as the subband keywords ``validation_rir_A`` /
        ``validation_rir_B`` do: evaluation_hops(), evaluation_totals(), predicted_pressure(), reset_evaluation() and
        evaluation.metrics() work the same, get_state() gains ``evaluation_history`` and ``evaluation_totals``.  ``ranks``: the
        evaluated ranks, a strictly ascending subset of the ranks the object emits (1..number_of_eigenvectors; in the MATLAB dialect
        the entries of number_of_eigenvectors); None: all of them.  Histories start from silence and totals from zero here.
        process_signal evaluates a whole group of hops per launch.  Outputs, filters and every other state are untouched.
        enable_evaluation_spectra(), after this call, adds the per-bin energies."""
        if self.mode != "broadband":
            raise RuntimeError("enable_evaluation() is the broadband mode's switch: in subband mode pass validation_rir_A and "
                               "validation_rir_B (and evaluation_ranks) to the constructor")
        if self.__dict__.get("_bb_evaluation") is not None:
            raise RuntimeError("enable_evaluation(): this object has its evaluation stage already")
        a, b = self._check_validation_rirs(validation_rir_A, validation_rir_B, self.number_of_srcs)
        if a.shape[0] > 20465:
            raise ValueError("validation_rir_*: Pv <= 20465 (one loudspeaker's window of Pv - 1 + 16 float64 samples has to fit "
                             "160 KB of LDS)")
        r = self._check_rank_subset(ranks, self._ranks, "ranks must be None or a strictly ascending list of ranks the object emits: "
                                    f"{list(self._ranks)}")
        self._eng.bb_set_evaluation(a, b, r)
        self._bb_evaluation = (a, b, r)
        self._bb_eval_hops = 0              # hops in the record of the last call

    def enable_evaluation_spectra(self):
        """Broadband mode: switch the per-bin spectra of the evaluation stage on, after enable_evaluation(), once, at any hop
        boundary.  From here on the device keeps the last block_size pressure samples of every pressure set and microphone and,
        after every hop, transforms them under the stream's sine window and accumulates |P|^2 per bin, as the subband keyword
        ``evaluation_spectra=True`` does: evaluation_spectra() and evaluation.spectral_metrics() work the same, get_state() gains
        ``evaluation_spectra`` (Z, 3 E + 1, K, Mv) and ``evaluation_ring`` (Z, 2 E + 1, Mv, N), reset_evaluation() zeroes both.
        Ring and spectra start from zero here.  process_signal transforms a whole group of hops per launch; the bits are those
        of the hop loop.  Everything else the object computes is untouched.  enable_evaluation_detectability(), after this call,
        adds the masking model's detectability of error and leakage on the same spectra."""
        if self.mode != "broadband":
            raise RuntimeError("enable_evaluation_spectra() is the broadband mode's switch: in subband mode pass "
                               "evaluation_spectra=True to the constructor")
        if self.__dict__.get("_bb_evaluation") is None:
            raise RuntimeError("enable_evaluation_spectra() comes after enable_evaluation()")
        if self.__dict__.get("_bb_evaluation_spectra"):
            raise RuntimeError("enable_evaluation_spectra(): this object keeps its evaluation spectra already")
        self._eng.bb_set_evaluation_spectra()
        self._bb_evaluation_spectra = True
        self._bb_spec_hops = 0              # hops since the switch: evaluation_spectra() is None before the first

    def enable_evaluation_detectability(self):
        """Broadband mode: switch the perceptual detectability of the evaluated pressures on, after
        enable_evaluation_spectra(), once, at any hop boundary.  From here on the device evaluates, behind the spectra of every
        hop, the second half of the masking model as the subband keyword ``evaluation_detectability=True`` does -- "error", the
        reproduction error masked by the program the listener wants, and "leak", the other program's leakage masked by this
        zone's own target (the threshold in quiet with one program), D = 1 just audible: evaluation_detectability(),
        evaluation_detectability_hops() and evaluation.detectability_metrics() work the same, get_state() gains
        ``evaluation_detectability`` (Z, 6 E + 1, Mv), reset_evaluation() zeroes it.  The tables are
        PerceptualTables(block_size, sampling_rate, fullscale_db_spl) -- ``self.model`` with perceptual=True -- and are kept as
        ``detectability_model``; a block they cannot be calibrated for raises what they raise and leaves the object as it was.
        Totals start from zero here.  process_signal evaluates a whole group of hops in three launches; the bits are those of the
        hop loop.  Everything else the object computes is untouched."""
        if self.mode != "broadband":
            raise RuntimeError("enable_evaluation_detectability() is the broadband mode's switch: in subband mode pass "
                               "evaluation_detectability=True to the constructor")
        if self.__dict__.get("_bb_evaluation") is None or not self.__dict__.get("_bb_evaluation_spectra"):
            raise RuntimeError("enable_evaluation_detectability() comes after enable_evaluation_spectra()")
        if self.__dict__.get("_bb_evaluation_detectability"):
            raise RuntimeError("enable_evaluation_detectability(): this object keeps its detectabilities already")
        tables = self.__dict__.get("model") if self.__dict__.get("perceptual") else None
        if tables is None:
            from .perceptual import PerceptualTables
            tables = PerceptualTables(self.block_size, self.sampling_rate, self._fullscale_db_spl)
        self._eng.bb_set_evaluation_detectability(tables)
        self.detectability_model = tables
        self._bb_evaluation_detectability = True
        self._detect_hops = 0               # hops the totals cover: since the switch, reset_evaluation() or a restored state
        self._bb_detect_rec = 0             # hops in the record of the last call; None from the accessors before the first

    @staticmethod
    def _eval_split(e, E):
        """(..., Z, 3 E + 1, Mv) -> the dict of bright, dark, error (..., Z, E, Mv) and target (..., Z, Mv)."""
        return {"bright": np.ascontiguousarray(e[..., :E, :]), "dark": np.ascontiguousarray(e[..., E:2 * E, :]),
                "error": np.ascontiguousarray(e[..., 2 * E:3 * E, :]), "target": np.ascontiguousarray(e[..., 3 * E, :])}

    def evaluation_hops(self):
        """Energies per hop of the last process_input_buffers / process_signal call: "bright", "dark", "error" (n, Z, E, Mv) and
        "target" (n, Z, Mv): n hops, Z zone programs that run (A first), E evaluated ranks.  None before the first hop."""
        Z, E, _, Mv = self._eval_dims()
        if self._hops == 0:
            return None
        if self.mode == "broadband":
            n = self._bb_eval_hops
            return self._eval_split(self._eng.bb_get_state("eval_hops", (n, Z, 3 * E + 1, Mv)), E) if n else None
        n = self._eng.state_bytes("eval_hops") // (8 * Z * (3 * E + 1) * Mv)
        if n == 0:
            return None
        return self._eval_split(self._eng.get_state("eval_hops", (n, Z, 3 * E + 1, Mv), np.float64), E)

    def evaluation_totals(self):
        """The energies summed over every hop since construction, set_state or reset_evaluation(): "bright", "dark", "error"
        (Z, E, Mv), "target" (Z, Mv); evaluation.metrics() turns them into NMSE and contrast.  None before the first hop."""
        Z, E, _, Mv = self._eval_dims()
        if self._hops == 0:
            return None
        if self.mode == "broadband":
            return self._eval_split(self._eng.bb_get_state("eval_totals", (Z, 3 * E + 1, Mv)), E)
        return self._eval_split(self._eng.get_state("eval_totals", (Z, 3 * E + 1, Mv), np.float64), E)

    def predicted_pressure(self):
        """Pressures of the last hop at the validation microphones: "bright" (own zone's microphones) and "dark" (the other
        zone's) (Z, E, H, Mv), "target" (the target output at the own zone's) (Z, H, Mv).  None before the first hop."""
        Z, E, _, Mv = self._eval_dims()
        if self._hops == 0:
            return None
        if self.mode == "broadband":
            if not self._bb_eval_hops:
                return None                   # enabled or resumed, no hop since
            p = self._eng.bb_get_state("eval_pressure", (Z, 2 * E + 1, self.hop_size, Mv))
        else:
            p = self._eng.get_state("eval_pressure", (Z, 2 * E + 1, self.hop_size, Mv), np.float64)
        return {"bright": np.ascontiguousarray(p[:, :E]), "dark": np.ascontiguousarray(p[:, E:2 * E]),
                "target": np.ascontiguousarray(p[:, 2 * E])}

    def evaluation_spectra(self):
        """The per-bin energies summed over every hop since construction, set_state or reset_evaluation(): "bright", "dark",
        "error" (Z, E, Mv, K) and "target" (Z, Mv, K), K = block_size / 2 + 1; evaluation.spectral_metrics() turns them into
        contrast and NMSE per bin or band.  None before the first hop."""
        Z, E, _, Mv = self._eval_dims()
        if self.__dict__.get("mode") == "broadband":
            if not self.__dict__.get("_bb_evaluation_spectra"):
                raise RuntimeError("this object keeps no evaluation spectra: call enable_evaluation_spectra()")
            if self._hops == 0 or not self._bb_spec_hops:
                return None                   # switched on, no hop since
            t = self._eng.bb_get_state("eval_spectra", (Z, 3 * E + 1, self._K, Mv))
        else:
            if not self.__dict__.get("_evaluation_spectra"):
                raise RuntimeError("this object keeps no evaluation spectra: pass evaluation_spectra=True")
            if self._hops == 0:
                return None
            t = self._eng.get_state("eval_spectra", (Z, 3 * E + 1, self._K, Mv), np.float64)
        # the device accumulates bins before microphones (neighbouring threads along the microphones)
        t = t.transpose(0, 1, 3, 2)
        return {"bright": np.ascontiguousarray(t[:, :E]), "dark": np.ascontiguousarray(t[:, E:2 * E]),
                "error": np.ascontiguousarray(t[:, 2 * E:3 * E]), "target": np.ascontiguousarray(t[:, 3 * E])}

    def _detect_dims(self):
        Z, E, _, Mv = self._eval_dims()
        if self.__dict__.get("mode") == "broadband":
            if not self.__dict__.get("_bb_evaluation_detectability"):
                raise RuntimeError("this object keeps no detectabilities: call enable_evaluation_detectability()")
        elif not self.__dict__.get("_evaluation_detectability"):
            raise RuntimeError("this object keeps no detectabilities: pass evaluation_detectability=True")
        return Z, E, Mv

    def _detect_state(self, name, shape):
        """a state array of the detectability stage; in broadband mode None while no hop has run since the switch"""
        if self._hops == 0:
            return None
        if self.mode == "broadband":
            return self._eng.bb_get_state(name, shape) if self._bb_detect_rec else None
        return self._eng.get_state(name, shape, np.float64)

    def evaluation_detectability(self):
        """Perceptual detectability D of the evaluated pressures (D = 1: just audible) over every hop since construction, set_state
        or reset_evaluation(): "error" -- the reproduction error in the bright zone, masked by the program the listener wants --
        and "leak" -- the other program's leakage, masked by this zone's own target -- as sums over the hops (Z, E, Mv),
        "error_max" / "leak_max" the largest hop, "error_audible" / "leak_audible" the number of hops with D > 1 (int64), and
        "hops", the hops counted; evaluation.detectability_metrics() turns them into means and audible shares.  None before the
        first hop."""
        Z, E, Mv = self._detect_dims()
        t = self._detect_state("eval_detect", (Z, 2, 3, E, Mv))
        if t is None:
            return None
        out = {"hops": int(self._detect_hops)}
        for i, name in enumerate(("error", "leak")):
            out[name] = np.ascontiguousarray(t[:, i, 0])
            out[name + "_max"] = np.ascontiguousarray(t[:, i, 1])
            out[name + "_audible"] = t[:, i, 2].astype(np.int64)
        return out

    def evaluation_detectability_hops(self):
        """The detectabilities per hop of the last process_input_buffers / process_signal call: "error" and "leak" (n, Z, E, Mv).
        None before the first hop."""
        Z, E, Mv = self._detect_dims()
        if self._hops == 0:
            return None
        if self.mode == "broadband":
            n = self._bb_detect_rec         # the host knows the hops of the last call
        else:
            n = self._eng.state_bytes("eval_detect_hops") // (8 * Z * 2 * E * Mv)
        if n == 0:
            return None
        r = self._detect_state("eval_detect_hops", (n, Z, 2, E, Mv))
        return {"error": np.ascontiguousarray(r[:, :, 0]), "leak": np.ascontiguousarray(r[:, :, 1])}

    def reset_evaluation(self):
        """Totals to zero and the output histories to silence: the next hop's totals are its own energies.  With
        evaluation_spectra=True, or after enable_evaluation_spectra() in broadband mode, the per-bin energies and the pressure ring
        too, with evaluation_detectability=True its totals.  After enable_evaluation_detectability() in broadband mode the
        detectability totals and their hop count go to zero as well."""
        self._eval_dims()
        if self.mode == "broadband":
            self._eng.bb_reset_evaluation()
            self._detect_hops = 0
            return
        self._eng.reset_evaluation()
        self._detect_hops = 0

    # ---- responses and mu, reassignable between hops (the reference reads them on every hop, apvast.py:161, 167-193) ----
    def _init_responses(self, rir_A, rir_B):
        """Read-only float64 copies of the constructor's responses and the targets built from them (apvast.py:100-112)."""
        P, L, M = self.rir_length, self.number_of_srcs, self.number_of_mics
        d = self.modeling_delay
        live = {"rir_A": np.array(rir_A, dtype=np.float64), "rir_B": np.array(rir_B, dtype=np.float64),
                "target_rir_A": np.zeros((P, M)), "target_rir_B": np.zeros((P, M))}
        for z, ref in (("A", self.reference_index_A), ("B", self.reference_index_B)):
            if 0 <= d < P and 0 <= ref < L:
                live["target_rir_" + z][d:] = live["rir_" + z][: P - d, ref, :]
        for a in live.values():
            a.flags.writeable = False
        self._live = live
        self._live_pending = set()          # names assigned since the last hop, applied together at the next one
        self._mu_pending = False
        self._live_applied = False          # some update reached the device: get_state carries the correction tails

    def _set_response(self, name, value):
        P, L, M = self.rir_length, self.number_of_srcs, self.number_of_mics
        shape = (P, L, M) if name.startswith("rir_") else (P, M)
        a = np.array(value, dtype=np.float64)
        if a.shape != shape:
            raise ValueError(f"{name} must have shape {shape} (the constructor's), got {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"{name} must be finite")
        if np.array_equal(a, self._live[name]):
            return
        a.flags.writeable = False
        self._live[name] = a
        self._live_pending.add(name)

    def _apply_live(self):
        """Everything assigned since the last hop, in one upload and one correction launch (apv_stream_set_rirs / apv_bb_set_rirs)."""
        if self._live_pending:
            new = {k: (self._live[k] if k in self._live_pending else None) for k in ("rir_A", "rir_B", "target_rir_A", "target_rir_B")}
            set_rirs = self._eng.bb_set_rirs if self.mode == "broadband" else self._eng.stream_set_rirs
            set_rirs(self.rir_length, **new)
            self._live_pending.clear()
            self._live_applied = True
        if self._mu_pending:
            self._eng.set_mu(self._mu)
            self._mu_pending = False
        if self._span_pending:
            self._eng.set_span(**self._span_args())
            self._span_pending = False
        if self._effort_pending:
            self._eng.set_effort_limit(self._effort_table())
            self._effort_pending = False
        if self._validation_pending:
            self._eng.set_validation_span(self._validation_floor_table())
            self._validation_pending = False

    # rir_A / rir_B (rir_length, L, M) and target_rir_A / target_rir_B (rir_length, M): an assignment between two hops takes effect at
    # the next one as lfilter(..., zi=state) makes it in the reference -- the samples already in take the old response's tail with
    # them.  Targets are not re-derived from new rir_* (apvast.py:100-112 builds them once).  The arrays held are read-only copies.
    rir_A = property(lambda self: self._live["rir_A"], lambda self, v: self._set_response("rir_A", v))
    rir_B = property(lambda self: self._live["rir_B"], lambda self, v: self._set_response("rir_B", v))
    target_rir_A = property(lambda self: self._live["target_rir_A"], lambda self, v: self._set_response("target_rir_A", v))
    target_rir_B = property(lambda self: self._live["target_rir_B"], lambda self, v: self._set_response("target_rir_B", v))

    @property
    def mu(self):
        return self._mu

    @mu.setter
    def mu(self, value):
        m = float(value)
        if not np.isfinite(m):
            raise ValueError("mu must be finite")
        if m != self._mu:
            self._mu = m
            self._mu_pending = True

    # ---- broadband mode: the reference's own time-domain algorithm, float64 on the device ----------
    def _init_broadband(self, device, seed):
        L, M, N, H = self.number_of_srcs, self.number_of_mics, self.block_size, self.hop_size
        J, S = int(self.filter_length), int(self.statistics_buffer_length)
        matlab = self.dialect == "matlab"
        if matlab:
            # apVast.m: a vector of ranks, one solution per entry (527-549); hop fixed to half a block (138); loading
            # relative to the spectral norm, bright 1e-8 and dark 5e-3 (552-569); zero initial buffers (175-180).
            # Indices stay 0-based here (make_python_test.m:9-10 passes 7 where Python takes 6).
            self._ranks = [int(v) for v in np.atleast_1d(self.number_of_eigenvectors)]
            if H * 2 != N:
                raise ValueError("MATLAB dialect: the hop is half a block (apVast.m:138)")
            reg = dict(reg_mode=_capi.REG_REL, reg_dark=5e-3, reg_bright=1e-8)
        else:
            self._ranks = list(range(1, int(self.number_of_eigenvectors) + 1))
            if EXPERIMENTAL_REGULARIZATION:
                reg = dict(reg_mode=_capi.REG_ABS, reg_dark=1e-7)                 # apvast.py:22-24
            else:
                reg = dict(reg_mode=_capi.REG_REL, reg_dark=1e-8)                 # apvast.py:26-27: B + 1e-8 ||B||_2 I
        V = len(self._ranks)
        self._K = N // 2 + 1
        zones = (1 if self.run_A else 0) | (2 if self.run_B else 0)
        self._eng = _capi.Engine(self._K, L, M, ranks=(1,), mu=self._mu, compute_dtype="f64", device=device, block_size=N,
                                 hop_size=H, n_zones=zones, dialect=self.dialect, max_sweeps=self._max_sweeps,
                                 out_layout=1,     # the device emits (hop, loudspeaker) arrays: nothing to transpose here
                                 **reg)
        self._eng.bb_set_rank_list(self._ranks if matlab else [])
        self._eng.bb_init(self.rir_A, self.rir_B, self.reference_index_A, self.reference_index_B, self.modeling_delay,
                          J, S, max(self._ranks))
        self._n_out = (int(self.run_A) + int(self.run_B)) * V * L + 2 * L
        if self.perceptual:
            from .perceptual import PerceptualTables
            self.model = PerceptualTables(N, self.sampling_rate, self._fullscale_db_spl)
            self._eng.bb_set_perceptual(self.model, self.dialect)             # apvast.py:322-324 / apVast.m:396-406
        if not matlab:
            rs = np.random if seed is None else np.random.RandomState(seed)  # apvast.py:124-129
            resp = [1e-3 * rs.randn(N, L, M) for _ in range(4)]
            tresp = [1e-3 * rs.randn(N, M) for _ in range(2)]
            self.set_state({"response": np.stack(resp), "target_response": np.stack(tresp)})
        self._hops = 0
        self._bb_cache = None
        self._bb_evaluation = None          # enable_evaluation() switches the stage on
        self._bb_eval_hops = 0
        self._bb_evaluation_spectra = False # enable_evaluation_spectra() switches the per-bin spectra on
        self._bb_spec_hops = 0
        self._bb_evaluation_detectability = False   # enable_evaluation_detectability() switches the detectability on
        self.detectability_model = None     # the tables the device received there
        self._detect_hops = self._bb_detect_rec = 0

    def _refresh_broadband(self):
        """A hop has run: what the attributes hold is stale.  Nothing is fetched here (see _bb_fetch)."""
        self._hops += 1
        self._bb_cache = {}

    def _bb_fetch(self, name):
        """Broadband attributes of the last hop, fetched from the device when first read (apvast.py:368-403)."""
        c = self._bb_cache
        if c is None or self._hops == 0:
            return None
        if name in c:
            return c[name]
        e, V, n = self._eng, len(self._ranks), self.filter_length * self.number_of_srcs
        if name.startswith("R_"):
            # R_X_to_Y belongs to the zone program of its SIGNAL X (apvast.py:333-347, 369-371): R_A_to_B exists whenever run_A is set
            path = {"R_A_to_A": 0, "R_A_to_B": 2, "R_B_to_B": 1, "R_B_to_A": 3}[name]
            if not (self.run_A, self.run_B)[path & 1]:
                return None
            v = e.bb_get_state(f"R{path}", (n, n))
            c[name] = v
            return v
        zone = {"A": 0, "B": 1}.get(name[-1])
        if zone is not None and not (self.run_A, self.run_B)[zone] and not name.startswith("input_spectrum"):
            return None
        if name.startswith("lambda_"):
            v = e.bb_get_state("lambda", (2, n))[zone].copy()                 # apvast.py:385-387
        elif name.startswith("w_"):
            v = e.bb_get_state("w", (2, V, n))[zone][:, :, None].copy()       # (V, n, 1), apvast.py:393, 398
        elif name.startswith("r_"):
            v = e.bb_get_state("r", (2, n))[zone][:, None].copy()
        elif name.startswith("input_spectrum_"):
            spec = e.bb_get_state("input_spectrum", (2, self._K, 2))
            v = (spec[zone, :, 0] + 1j * spec[zone, :, 1]).reshape(-1, 1)     # apvast.py:430-431
        else:
            raise AttributeError(name)
        c[name] = v
        return v

    # ---- per-hop call (apvast.py:153-165) -------------------------------------------------
    def process_input_buffers(self, input_A, input_B):
        input_A = np.asarray(input_A)
        input_B = np.asarray(input_B)
        if input_A.size != self.hop_size or input_B.size != self.hop_size:
            raise RuntimeError("invalid input size")                          # apvast.py:154-155
        self._apply_live()
        if self.mode == "broadband":
            out = self._eng.bb_process_block(input_A, input_B, self._n_out)      # (groups, H, L), fresh for every hop
            res = self._split_groups(out)
            self._bb_eval_hops = self._bb_spec_hops = 1
            if self._bb_evaluation_detectability:
                self._bb_detect_rec = 1
                self._detect_hops += 1
            self._refresh_broadband()
            return res
        out = self._eng.process_block(input_A, input_B, self._n_out)         # (groups, H, L): one (H, L) array per zone and rank
        if out.dtype != np.float64:
            out = out.astype(np.float64)
        res = self._split_groups(out)
        self._detect_hops += 1
        self._refresh_attributes()
        return res

    def process_signal(self, input_A, input_B, out=None):
        """Every hop of two whole signals in one call: the hop loop of main.m:52-62 / make_python_test.m:44-51 around
        process_input_buffers, with consecutive hops pipelined on the device (subband mode) or their joint
        diagonalisations solved as one batch (broadband mode).  Returns
        (output_A, output_B, target_A, target_B): per zone a list over the ranks of (n_samples, L) arrays, None for a
        zone that does not run; sample for sample what the per-hop calls return, concatenated.  The attributes
        afterwards are those of the last hop.
        `out`: optional C-contiguous array of shape signal_output_shape(n_samples) and dtype signal_output_dtype to receive
        the samples (the returned arrays are then slices of it, in its dtype: float32 for dtype="f32" / "mixed").  A 10 s signal returns 184 MB; a caller that processes many
        signals saves the first-touch cost of that much fresh memory by passing the same array again."""
        input_A = np.asarray(input_A).ravel()
        input_B = np.asarray(input_B).ravel()
        if input_A.size != input_B.size or input_A.size % self.hop_size:
            raise RuntimeError("invalid input size")
        if input_A.size == 0:
            raise RuntimeError("invalid input size")
        self._apply_live()
        if self.mode == "broadband":
            # the joint diagonalisations of up to 16 consecutive hops are solved as one batch (apv_bb_process_signal); the library
            # writes (groups, n_samples, L) -- every zone program's and rank's whole signal as the array handed out below
            out = self._eng.bb_process_signal(input_A, input_B, self._n_out, out=out)
            res = self._split_groups(out)
            self._bb_eval_hops = self._bb_spec_hops = input_A.size // self.hop_size
            if self._bb_evaluation_detectability:
                self._bb_detect_rec = input_A.size // self.hop_size
                self._detect_hops += input_A.size // self.hop_size
            self._hops += input_A.size // self.hop_size - 1
            self._refresh_broadband()
            return res
        given = out is not None
        out = self._eng.process_signal(input_A, input_B, self._n_out, out=out)   # (groups, n_samples, L), written in place by the library
        # float32 / mixed arithmetic produce float32 samples: a fresh result is widened to the float64 the reference returns; a
        # caller's own `out` is handed back as it is (its slices), without a second copy of the whole signal on the host
        if out.dtype != np.float64 and not given:
            out = out.astype(np.float64)
        res = self._split_groups(out)
        self._detect_hops += input_A.size // self.hop_size
        self._refresh_attributes()
        return res

    @property
    def signal_schedule(self):
        """How the last process_signal call of a subband stream ran: (hops that went through the chunked schedule -- a chunk of
        hops per launch --, hops that went hop by hop).  (0, 0) before the first such call; process_input_buffers does not change
        it.  Read-only, and no part of get_state() / set_state().  Broadband mode has no such schedule: None."""
        if self.mode == "broadband":
            return None
        c, p = self._eng.get_state("signal_schedule", (2,), np.int32)
        return int(c), int(p)

    def signal_output_shape(self, n_samples):
        """Shape of process_signal's `out`: (zones x ranks + 2 target paths, n_samples, L)."""
        return (self._n_out // self.number_of_srcs, int(n_samples), self.number_of_srcs)

    def alloc_signal_output(self, n_samples):
        """An array for process_signal's `out` in page-locked host memory: the device writes the samples into it by DMA while it
        computes the next hops (broadband mode at the reference's test parameters returns 5.2 MB a hop: a pageable array costs a
        second pass over all of it on the host).  Falls back to an ordinary array when the runtime refuses the allocation."""
        shape, dt = self.signal_output_shape(n_samples), self.signal_output_dtype
        arr = self._eng.pinned_empty(shape, dt)
        return arr if arr is not None else np.empty(shape, dtype=dt)

    @property
    def signal_output_dtype(self):
        return np.float64 if self.mode == "broadband" else self._eng.s_dtype

    def _split_groups(self, out):
        """out: (groups, samples, L) with the groups [zone A: rank 1..V][zone B: rank 1..V][A_t][B_t] (zones that run) ->
        (A, B, A_t, B_t) as the reference returns them (apvast.py:498-506): per zone a list over the ranks of (samples, L)
        arrays -- slices of `out`, which is fresh for every call -- None for a zone that does not run (apvast.py:433-443)."""
        V = len(self._ranks)
        g, res = 0, []
        for run in (self.run_A, self.run_B):
            if run:
                res.append([out[g + i] for i in range(V)])
                g += V
            else:
                res.append(None)
        for _ in range(2):
            # the same target filter at every rank (apvast.py:389-390, 418-422): the V entries are ONE read-only array (V copies
            # were 5 MB a hop at the reference's test parameters; a caller that wants to write into one takes a copy)
            t = out[g]
            t.flags.writeable = False
            res.append([t] * V)
            g += 1
        return tuple(res)

    def _refresh_attributes(self):
        """A hop (or a whole signal) has run: drop what was fetched for the previous one.  Nothing crosses PCIe here: w_*,
        lambda_*, input_spectrum_*, filter_spectra_* (and U_*, R_*, r_*) are fetched when they are read (_sb_fetch)."""
        self._hops += 1
        self._sb_cache = {}

    def _sb_fetch(self, name):
        """Subband attributes of the last hop (leading bin axis), fetched from the device when first read."""
        if self._hops == 0:
            return None
        c = self._sb_cache
        if name in c:
            return c[name]
        e, K, L, V = self._eng, self._K, self.number_of_srcs, len(self._ranks)
        z = name[-1]
        if name.startswith("input_spectrum_"):
            spec = e.get_state("input_spectrum", (2, K), e.sc_dtype)
            c["input_spectrum_A"] = spec[0].astype(np.complex128).reshape(-1, 1)   # apvast.py:430-431
            c["input_spectrum_B"] = spec[1].astype(np.complex128).reshape(-1, 1)
            return c[name]
        if not (self.run_A if z == "A" else self.run_B):
            return None
        if (name.startswith("w_") and not name.startswith("w_time_")) or name.startswith("filter_spectra_"):
            w = e.get_state("w_" + z, (K, V, L), e.w_dtype).astype(np.complex128)
            c["w_" + z] = np.ascontiguousarray(w.transpose(1, 0, 2))               # (V, K, L)
            c["filter_spectra_" + z] = [c["w_" + z][i] for i in range(V)]          # V x (K, L): the filters ARE the spectra
        elif name.startswith("w_time_"):
            if not self.constrain_filter_length:
                return None
            c[name] = e.get_state(name, (V, int(self.filter_length), L), e.lam_dtype).astype(np.float64)
        elif name.startswith("lambda_"):
            c[name] = e.get_state(name, (K, L), e.lam_dtype).astype(np.float64)
        else:
            raise AttributeError(name)
        return c[name]

    @property
    def not_converged(self):
        """Hops so far in which some bin's eigen-iteration stopped at its sweep cap (each of them warned)."""
        return self._eng.stream_not_converged()

    # ---- attributes the reference sets every hop, fetched from the device when read ------------------------
    def _bb_filter_spectra(self):
        if "fs" not in self._bb_cache:
            K, L, V = self._K, self.number_of_srcs, len(self._ranks)
            fs = self._eng.bb_get_state("filter_spectra", (self._n_out, K, 2))
            fs = fs[..., 0] + 1j * fs[..., 1]                                     # [n_out][K], channel (v, l)
            out, pos = {}, 0
            for z, run in (("A", self.run_A), ("B", self.run_B)):
                if run:
                    out[z] = [np.ascontiguousarray(fs[pos + v * L: pos + (v + 1) * L].T) for v in range(V)]    # V x (K, L)
                    pos += V * L
            for z in ("A_t", "B_t"):
                t = np.ascontiguousarray(fs[pos: pos + L].T)
                out[z] = [t.copy() for _ in range(V)]                             # the same target filter at every rank
                pos += L
            self._bb_cache["fs"] = out
        return self._bb_cache["fs"]

    def _subband_stats(self, zone):
        key = ("stats", zone)
        if key not in self._sb_cache:
            self._sb_cache[key] = self._eng.stream_statistics(zone)
        return self._sb_cache[key]

    def _zone_attr(self, z, what):
        """U / R_bright / R_dark / r of zone program z ('A' | 'B'); None for a zone that does not run."""
        zi = "AB".index(z)
        if not (self.run_A, self.run_B)[zi] or self._hops == 0:
            return None
        if self.mode == "broadband":
            n = self.filter_length * self.number_of_srcs
            if what == "U":
                key = ("U", zi)
                if key not in self._bb_cache:
                    self._bb_cache[key] = self._eng.bb_get_state(f"U{zi}", (n, n))
                return self._bb_cache[key]
            raise AttributeError(what)
        RB, RD, r, U, _ = self._subband_stats(zi)
        return {"U": U, "RB": RB, "RD": RD, "r": r}[what]

    # per-bin (subband mode: (K, L, L) complex128, recomputed in float64 from the hop's control-point spectra) or
    # (J L) x (J L) real (broadband mode) eigenvectors of the last hop, columns in descending order   apvast.py:380-382
    U_A = property(lambda self: self._zone_attr("A", "U"))
    U_B = property(lambda self: self._zone_attr("B", "U"))

    _LAZY = ("w_A", "w_B", "lambda_A", "lambda_B", "input_spectrum_A", "input_spectrum_B", "filter_spectra_A", "filter_spectra_B",
             "R_A_to_A", "R_A_to_B", "R_B_to_B", "R_B_to_A", "r_A", "r_B", "w_time_A", "w_time_B")

    def __getattr__(self, name):
        # the attributes the reference assigns in every hop (apvast.py:368-403): read from the device on demand, cached until
        # the next hop; plain attribute access for everything else
        d = self.__dict__
        if name in apvast._LAZY and "_eng" in d and "_hops" in d:
            if d.get("mode") == "broadband":
                if name.startswith("w_time_"):
                    return None                                                   # broadband w_* are the J-tap filters themselves
                if name.startswith("filter_spectra_"):
                    if d["_hops"] == 0:
                        return None
                    fs = self._bb_filter_spectra()
                    return fs.get(name[len("filter_spectra_"):])                  # None: that zone does not run (apvast.py:391-400)
                return self._bb_fetch(name)
            sub = {"R_A_to_A": ("A", "RB"), "R_A_to_B": ("A", "RD"), "R_B_to_B": ("B", "RB"), "R_B_to_A": ("B", "RD"),
                   "r_A": ("A", "r"), "r_B": ("B", "r")}
            if name in sub:
                return self._zone_attr(*sub[name])
            return self._sb_fetch(name)
        if name in ("filter_spectra_A_t", "filter_spectra_B_t") and d.get("mode") == "broadband" and d.get("_hops", 0) > 0:
            return self._bb_filter_spectra()[name[len("filter_spectra_"):]]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    # ---- checkpoint / fixtures -----------------------------------------
    _BB_STATE = ("response", "target_response", "stats", "target_stats", "overlap", "target_overlap", "input_block",
                 "input_history", "out_overlap")
    _SB_STATE = ("response", "target_response", "input_block", "input_history", "out_overlap")
    _LIVE_STATE = ("fir_correction", "target_fir_correction")       # present once a response update has been applied
    _WIN_STATE = ("statistics_window", "statistics_window_fill")    # present with statistics_hops > 1
    _FORGET_STATE = ("statistics_forgetting_sums",)                  # present with statistics_forgetting set
    _FIR_STATE = ("fir_synthesis_taps", "fir_synthesis_history")    # present with synthesis="fir"
    _EVAL_STATE = ("evaluation_history", "evaluation_totals")       # present with validation_rir_A / validation_rir_B
    _EVALSPEC_STATE = ("evaluation_spectra", "evaluation_ring")     # present with evaluation_spectra=True
    _EVALDETECT_STATE = ("evaluation_detectability",)               # present with evaluation_detectability=True

    def get_state(self):
        """Everything the next hop depends on (the reference's instance attributes of apvast.py:115-151), as float64 arrays
        in the reference's own axis order; ``b.set_state(a.get_state())`` makes b continue exactly as a would.  Once a response
        update has been applied, also the correction tails it left: ``fir_correction`` (4, rir_length - 1, L, M) and
        ``target_fir_correction`` (2, rir_length - 1, M).  The responses and mu are not state: an object resumed across an
        update must first be given the same rir_* / target_rir_* / mu (by construction or assignment) as the one it continues.
        With ``statistics_hops = T > 1`` also the window: ``statistics_window`` (zone programs that run, T, K, 2 L^2 + L) complex128
        -- per hop and bin [R_B (lower triangle) | R_D (lower triangle) | r] of that hop alone, hops oldest first, zeros beyond the
        fill level -- and ``statistics_window_fill``, the number of hops it holds (it fills during the first T - 1 hops).  Both are
        absent when T = 1.  With ``statistics_forgetting`` set, the running sums instead: ``statistics_forgetting_sums`` (zone
        programs that run, K, 2 L^2 + L), per bin [R_B (lower triangle) | R_D (lower triangle) | r], complex128 (complex64 with
        ``dtype="f32"`` up to 64 loudspeakers: the precision they are kept in); absent otherwise.  R_*, r_*, U_*, lambda_* are what the last hop of THIS object left on the device: they follow a restored
        window from the next hop on, not from set_state."""
        return {row.key: row.get(self) for row in self._STATE_ROWS if (row.reports or row.accepts)(self)}

    def set_state(self, state):
        rows = [row for row in self._STATE_ROWS if row.accepts(self)]
        known = [row.key for row in rows]
        unknown = sorted(set(state) - set(known))
        if unknown:
            raise KeyError(f"set_state: no such state array(s) in {self.mode} mode: {unknown}; known: {known}")
        rows = [row for row in rows if row.key in state]
        for row in rows:
            if row.shape is not None:
                want, got = row.shape(self), np.asarray(state[row.key]).shape
                if got != want:
                    raise ValueError(f"{row.key} must have shape {want}, got {got}")
        for row in rows:
            row.put(self, state[row.key])

    # What the rows of the table (_state_rows, below the class) are made of.  Real samples cross in float64: broadband mode keeps
    # them so, subband mode in the front-end's own precision (float32, or float64 with dtype="f64").
    def _get_real(self, name, shape):
        e = self._eng
        return e.bb_get_state(name, shape) if self.mode == "broadband" else e.get_state(name, shape, e.s_dtype).astype(np.float64)

    def _put_real(self, name, value):
        e = self._eng
        if self.mode == "broadband":
            e.bb_set_state(name, np.asarray(value, dtype=np.float64))
        else:
            e.set_state(name, np.asarray(value, dtype=e.s_dtype))

    def _get_banks(self, name, count, length):
        """the device's [M][L][len] of the four paths (count = 4) as (4, len, L, M), its [M][len] of the two targets as (2, len, M)"""
        shape = (self.number_of_mics,) + ((self.number_of_srcs,) if count == 4 else ()) + (length,)
        return np.stack([self._get_real(f"{name}{i}", shape).T for i in range(count)])

    def _put_banks(self, name, count, value):
        for i in range(count):
            self._put_real(f"{name}{i}", np.asarray(value)[i].T)

    def _put_live(self, name, count, value):
        self._apply_live()                 # responses assigned before the resume are in place before their tails are
        self._put_banks(name, count, value)
        self._live_applied = True

    def _zones(self):
        return [z for z, run in enumerate((self.run_A, self.run_B)) if run]

    def _get_zones(self, name, shape, dtype):
        """one engine array per zone program that runs ({z}: 0 / 1, {Z}: A / B), stacked"""
        return np.stack([self._eng.get_state(name.format(z=z, Z="AB"[z]), shape, dtype) for z in self._zones()])

    def _put_zones(self, name, value, dtype):
        for i, z in enumerate(self._zones()):
            self._eng.set_state(name.format(z=z, Z="AB"[z]), np.asarray(value)[i].astype(dtype))

    def _get_signals(self, name, length):
        """one engine array per input signal as (2, len); not fetched where len = 0"""
        return np.stack([self._get_real(f"{name}{g}", (length,)) if length else np.zeros(0) for g in range(2)])

    def _put_signals(self, name, value):
        a = np.asarray(value)
        for g in range(2 if a.size else 0):
            self._put_real(f"{name}{g}", a[g])

    def _input_history_len(self):
        # rir_length - 1 + hop_size samples; more in subband mode when the RIR convolution is uniformly partitioned (long responses)
        if self.mode == "broadband":
            return self.rir_length - 1 + self.hop_size
        return self._eng.state_bytes("input_history0") // np.dtype(self._eng.s_dtype).itemsize

    def _get_detectability(self):
        # the totals as the device keeps them -- per program sum, max and audible count of the error, then of the leak -- and
        # in a last row the hops they cover, which only the host counts
        Z, E, _, Mv = self._eval_dims()
        tot = (self._eng.bb_get_state("eval_detect", (Z, 6 * E, Mv)) if self.mode == "broadband"
               else self._eng.get_state("eval_detect", (Z, 6 * E, Mv), np.float64))
        return np.concatenate([tot,
                               np.full((Z, 1, Mv), float(self._detect_hops))], axis=1)

    def _put_detectability(self, value):
        a, E = np.asarray(value, dtype=np.float64), self._eval_dims()[1]
        hops = a[0, 6 * E, 0]
        if not (hops >= 0 and hops == np.floor(hops) and np.all(a[:, 6 * E] == hops)):
            raise ValueError("evaluation_detectability: the last row must hold one hop count, a non-negative integer")
        if self.mode == "broadband":
            self._eng.bb_set_state("eval_detect", np.ascontiguousarray(a[:, :6 * E]))
        else:
            self._eng.set_state("eval_detect", np.ascontiguousarray(a[:, :6 * E]))
        self._detect_hops = int(hops)

    def close(self):
        self._eng.close()


# One row per key of the state dict.  accepts(self): set_state takes the key; reports(self) (None: as accepts): get_state returns
# it; shape(self) (None: the device's size check is the only one): what set_state compares the value's shape with; get(self) -> the
# value; put(self, value).
_StateRow = collections.namedtuple("_StateRow", "key accepts reports shape get put")


def _state_rows():
    """The table, in the order set_state applies the keys."""
    always = lambda self: True
    bb = lambda self: self.mode == "broadband"
    sub = lambda on: (lambda self: self.mode == "subband" and bool(on(self)))         # a subband feature behind its keyword
    win, forget = sub(lambda self: self.statistics_hops > 1), sub(lambda self: self.statistics_forgetting is not None)
    fir, ev_sub = sub(lambda self: self.synthesis == "fir"), sub(lambda self: self._evaluation is not None)
    # the evaluation stage: the constructor's in subband mode, enable_evaluation()'s in broadband mode
    ev = lambda self: ev_sub(self) or (bb(self) and getattr(self, "_bb_evaluation", None) is not None)
    evs_sub, evd_sub = sub(lambda self: self._evaluation_spectra), sub(lambda self: self._evaluation_detectability)
    # the per-bin spectra: the constructor's keyword in subband mode, enable_evaluation_spectra()'s in broadband mode
    evs = lambda self: evs_sub(self) or (bb(self) and getattr(self, "_bb_evaluation", None) is not None
                                         and bool(getattr(self, "_bb_evaluation_spectra", False)))
    # the detectability: the constructor's keyword in subband mode, enable_evaluation_detectability()'s in broadband mode
    evd = lambda self: evd_sub(self) or (bb(self) and bool(getattr(self, "_bb_evaluation_detectability", False)) and bool(evs(self)))
    live = lambda self: self._live_applied
    N = lambda self: self.block_size
    S = lambda self: self.statistics_buffer_length
    Q = lambda self: max(self.rir_length - 1, 1)
    J = lambda self: int(self.filter_length)
    slot = lambda self: 2 * self.number_of_srcs ** 2 + self.number_of_srcs             # a bin's [R_B | R_D | r], lower triangles
    taps = lambda self: (len(self._ranks), J(self), self.number_of_srcs)
    dims = lambda f: (lambda self: f(self, *self._eval_dims()))                        # f(self, Z, E, Pv, Mv)

    def banks(key, count, length, accepts=always, reports=None, put=apvast._put_banks):
        """(4, len, L, M) of the four paths or (2, len, M) of the two targets; no shape check of its own"""
        return _StateRow(key, accepts, reports, None, lambda self: self._get_banks(key, count, length(self)),
                         lambda self, v: put(self, key, count, v))

    def real(key, shape):
        """one array of real samples under the key's own name; no shape check of its own"""
        return _StateRow(key, always, None, None, lambda self: self._get_real(key, shape(self)), lambda self, v: self._put_real(key, v))

    def zones(key, name, accepts, shape, dtype, out=None):
        """(zone programs that run, *shape) of a subband feature, kept in dtype(engine) and handed out as `out` (None: as kept)"""
        return _StateRow(key, accepts, None, lambda self: (len(self._zones()),) + shape(self),
                         lambda self: self._get_zones(name, shape(self), dtype(self._eng)).astype(out or dtype(self._eng)),
                         lambda self, v: self._put_zones(name, v, dtype(self._eng)))

    def whole(key, name, accepts, shape, dtype=lambda e: np.float64):
        """one engine array of a feature, handed out as float64 (what the broadband stream keeps); neither fetched nor sent where
        it has no elements"""
        def get(self):
            if not all(shape(self)):
                return np.zeros(shape(self))
            if bb(self):
                return self._eng.bb_get_state(name, shape(self))
            return self._eng.get_state(name, shape(self), dtype(self._eng)).astype(np.float64)

        def put(self, v):
            if not all(shape(self)):
                return
            if bb(self):
                self._eng.bb_set_state(name, np.ascontiguousarray(v, dtype=np.float64))
            else:
                self._eng.set_state(name, np.ascontiguousarray(v, dtype=dtype(self._eng)))
        return _StateRow(key, accepts, None, shape, get, put)

    return (
        banks("response", 4, N),
        banks("target_response", 2, N),
        banks("stats", 4, S, bb),
        banks("target_stats", 2, S, bb),
        banks("overlap", 4, N, bb),
        banks("target_overlap", 2, N, bb),
        real("input_block", lambda self: (2, N(self))),
        _StateRow("input_history", always, None, None, lambda self: self._get_signals("input_history", self._input_history_len()),
                  lambda self, v: self._put_signals("input_history", v)),
        real("out_overlap", lambda self: (self._n_out, N(self))),
        zones("statistics_window", "stat_window{z}", win, lambda self: (self.statistics_hops, self._K, slot(self)),
              lambda e: e.stat_dtype, out=np.complex128),
        _StateRow("statistics_window_fill", win, None, None, lambda self: int(self._eng.get_state("stat_window_fill", (1,), np.int32)[0]),
                  lambda self, v: self._eng.set_state("stat_window_fill", np.array([int(v)], dtype=np.int32))),
        zones("statistics_forgetting_sums", "stat_forget{z}", forget, lambda self: (self._K, slot(self)), lambda e: e.stat_dtype),
        zones("fir_synthesis_taps", "fir_synth_taps_{Z}", fir, taps, lambda e: e.lam_dtype, out=np.float64),
        _StateRow("fir_synthesis_history", fir, None, lambda self: (2, J(self) - 1),
                  lambda self: self._get_signals("fir_synth_history", J(self) - 1),
                  lambda self, v: self._put_signals("fir_synth_history", v)),
        # the newest Pv - 1 output samples of every evaluated group (zone programs that run; the E ranks, then the target)
        # and the accumulated energies [bright of the E ranks | dark | error | target]
        whole("evaluation_history", "eval_history", ev, dims(lambda self, Z, E, Pv, Mv: (Z, E + 1, Pv - 1, self.number_of_srcs)),
              dtype=lambda e: e.s_dtype),
        whole("evaluation_totals", "eval_totals", ev, dims(lambda self, Z, E, Pv, Mv: (Z, 3 * E + 1, Mv))),
        # the per-bin energies as the device keeps them and the last N pressure samples of every set, oldest first
        whole("evaluation_spectra", "eval_spectra", evs, dims(lambda self, Z, E, Pv, Mv: (Z, 3 * E + 1, self._K, Mv))),
        whole("evaluation_ring", "eval_ring", evs, dims(lambda self, Z, E, Pv, Mv: (Z, 2 * E + 1, Mv, N(self)))),
        _StateRow("evaluation_detectability", evd, None, dims(lambda self, Z, E, Pv, Mv: (Z, 6 * E + 1, Mv)),
                  apvast._get_detectability, apvast._put_detectability),
        # the two correction keys last: always taken, handed out once a response update has reached the device
        banks("fir_correction", 4, Q, reports=live, put=apvast._put_live),
        banks("target_fir_correction", 2, Q, reports=live, put=apvast._put_live),
    )


apvast._STATE_ROWS = _state_rows()
