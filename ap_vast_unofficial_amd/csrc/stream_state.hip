// Named state arrays of the subband stream: apv_state_bytes, apv_get_state, apv_set_state.  One table (resolve) says which names a
// stream has and where and how each is kept; the three entry points look a name up once and act on what they are told.
#include "stream_types.h"
#include "state_layout.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

// How a named array is kept, which is all the entry points need to know about it.
struct StateRef {
    enum Kind {
        None,       // no such name in this stream
        Plain,      // device array, as stored
        Ring,       // device ring of rows x len elements of esz bytes at the stream's ring offset: callers see logical order
        Grouped,    // control-point spectra in groups of xg bins, [Kp / xg][C][xg]: callers get bin-major [K][C] and cannot set them
        Live,       // pending correction tail `index` of a response update: apv_live_state's
        Window,     // statistics ring of `rows` slots of len elements: callers see the slots in the order of age, zeros beyond the fill
        Fill,       // the int32 fill level of that ring
        Host,       // host array, never set
    } kind = None;
    void* ptr = nullptr;
    size_t bytes = 0;
    size_t rows = 0, len = 0, esz = 0;
    int index = 0;
    bool read_only = false;   // a set is refused before its size is looked at
    bool get_only = false;    // a set does not know the name at all
    bool settle = false;      // the stream is synchronised before the copy as well as behind it
};

StateRef plain(void* p, size_t bytes) { StateRef r; r.kind = StateRef::Plain; r.ptr = p; r.bytes = bytes; return r; }
StateRef settled(StateRef r) { r.settle = true; return r; }
StateRef read_only(StateRef r) { r.read_only = true; return r; }
StateRef get_only(StateRef r) { r.get_only = true; return r; }
StateRef of_kind(StateRef::Kind kind, StateRef r) { r.kind = kind; return r; }
StateRef host(const void* p, size_t bytes) { return of_kind(StateRef::Host, plain(const_cast<void*>(p), bytes)); }
StateRef live_tail(int j, size_t bytes) { StateRef r = of_kind(StateRef::Live, plain(nullptr, bytes)); r.index = j; return r; }
StateRef rows_of(StateRef::Kind kind, void* p, size_t rows, size_t len, size_t esz) {
    StateRef r = of_kind(kind, plain(p, rows * len * esz));
    r.rows = rows; r.len = len; r.esz = esz;
    return r;
}

// The table.  Real samples are float32 (float64 with the float64 front-end: e1 bytes), spectra the matching complex type (e2);
// filters, eigenvalues and taps follow cfg.out_c128 (wz, lz); a row applies where its condition holds, and a name no row takes
// does not exist in this stream.
StateRef resolve(apv_handle* h, const char* name) {
    apv_stream* s = h->st;
    const size_t N = s->N, H = s->H, K = s->K, C = s->C, M = s->M, L = s->L, nV = s->nV, J = s->taps, e1 = s->esz, e2 = 2 * s->esz;
    const size_t wz = wsz(h), lz = lsz(h), Q = std::max(s->P - 1, 1);
    const size_t Z = s->ev_Z, E = s->ev_E, Mv = s->ev_Mv, sets = s->ev_sets, rec = s->ev_nrec;
    const size_t slot = apv_statwin_slot_elems(s->L), cz = s->win_c128 ? 16 : 8;      // a bin's [R_B | R_D | r] (lower triangles), complex
    const bool forget = s->fg_beta > 0.0, window = !forget && s->win_T > 1;
    const auto is = [&](const char* n) { return std::strcmp(name, n) == 0; };
    const auto idx = [&](const char* pre, int count, char first = '0') { return apv_name_index(name, pre, count, first); };
    int q;
    // the rings, [rows][N] in logical order
    if ((q = idx("response", 4)) >= 0) return rows_of(StateRef::Ring, s->resp[q], C, N, e1);
    if ((q = idx("target_response", 2)) >= 0) return rows_of(StateRef::Ring, s->tresp[q], M, N, e1);
    if (is("input_block")) return rows_of(StateRef::Ring, s->inblk, 2, N, e1);
    // [keep + H] samples of input signal g, keep = P - 1 (fir_np H where K1 is partitioned: apv_state_bytes tells); [n_out][N]
    if ((q = idx("input_history", 2)) >= 0) return plain(s->xhist[s->cur][q], (size_t)(s->keep + s->H) * e1);
    if (is("out_overlap")) return plain(s->outov, (size_t)s->n_out * N * e1);
    // the last hop's spectra: [K][C], [K][M], [2][K] complex; the perceptual weights [K][M] where the weighting is on
    if ((q = idx("spectra", 4)) >= 0) return of_kind(s->xg > 1 ? StateRef::Grouped : StateRef::Plain, plain(s->X[q], K * C * e2));
    if ((q = idx("target_spectra", 2)) >= 0) return plain(s->tspec[q], K * M * e2);
    if (is("input_spectrum")) return plain(s->inspec, 2 * K * e2);
    if ((q = idx("weights", 2)) >= 0 && s->nch > 0) return plain(s->Wgt[q], K * M * e1);
    // the last hop's filters [K][nV][L] c64 | c128 and eigenvalues [K][L] f32 | f64
    if ((q = idx("w_", 2, 'A')) >= 0) return plain(s->w[q], K * nV * L * wz);
    if ((q = idx("lambda_", 2, 'A')) >= 0) return plain(s->lam[q], K * L * lz);
    // [C][P - 1], [M][P - 1]: tails a response update (apv_stream_set_rirs) still has to add; zeros in a stream never updated
    if ((q = apv_live_index(name)) >= 0) return live_tail(q, e1 * (q < 4 ? C : M) * Q);
    // statistics window (apv_stream_set_stat_hops): [win_T][K][2 L^2 + L] complex of the ring's precision per zone program that
    // runs, and how many of the slots hold a hop
    if (window && (q = idx("stat_window", 2)) >= 0 && s->win_ring[q])
        return settled(rows_of(StateRef::Window, s->win_ring[q], s->win_T, K * slot, cz));
    if (window && is("stat_window_fill")) return settled(of_kind(StateRef::Fill, plain(s->win_ctr, sizeof(int32_t))));
    // forgetting statistics (apv_stream_set_stat_forgetting): the accumulator [K][2 L^2 + L] per zone program that runs
    if (forget && (q = idx("stat_forget", 2)) >= 0 && s->win_ring[q]) return settled(plain(s->win_ring[q], K * slot * cz));
    // {sum in ms, count} of the timed statistics launches of either (APV_STAT_WINDOW_TIMING): refused by a set after its size
    if ((window || forget) && is("stat_window_kernel_ms")) return settled(host(s->win_tm.ms, sizeof(s->win_tm.ms)));
    // filter-length constraint (apv_stream_set_filter_taps): [nV][J][L] f32 | f64, the taps of the last hop's projected filters, per
    // zone program that runs; {sum, count} of the timed projections (APV_FILTER_CONSTRAINT_TIMING)
    if ((q = idx("w_time_", 2, 'A')) >= 0 && s->wtaps[q]) return plain(s->wtaps[q], nV * J * L * lz);
    if (s->taps > 0 && is("filter_constraint_kernel_ms")) return get_only(host(s->cf_tm.ms, sizeof(s->cf_tm.ms)));
    // FIR synthesis (apv_stream_set_synthesis): [nV][J][L] taps the next hop fades from, the [J - 1] newest samples of input signal
    // g; {sum, count} of the timed launches (APV_FIR_SYNTHESIS_TIMING)
    if ((q = idx("fir_synth_taps_", 2, 'A')) >= 0 && s->fs_taps[q]) return plain(s->fs_taps[q], nV * J * L * lz);
    if (s->fir_synth && (q = idx("fir_synth_history", 2)) >= 0) return plain(s->fs_hist[s->cur][q], (J - 1) * e1);
    if (s->fir_synth && is("fir_synthesis_kernel_ms")) return get_only(host(s->fs_tm.ms, sizeof(s->fs_tm.ms)));
    // evaluation (apv_stream_set_evaluation, see include/apvast_hip.h): the last hop's pressures [sets][H][Mv], the energies
    // [Z][3 E + 1][Mv] of each hop of the last call and their totals, all f64; the [Z (E + 1)][Pv - 1][L] newest output samples
    if (s->ev_on && is("eval_pressure")) return read_only(plain(s->ev_p, 8 * sets * H * Mv));
    if (s->ev_on && is("eval_hops")) return read_only(plain(s->ev_rec, 8 * Z * (3 * E + 1) * Mv * rec));
    if (s->ev_on && is("eval_totals")) return plain(s->ev_tot, 8 * Z * (3 * E + 1) * Mv);
    if (s->ev_on && is("eval_history")) return plain(s->ev_hist[s->cur], (size_t)s->ev_nhist * (s->ev_Pv - 1) * L * e1);
    // its per-bin spectra (apv_stream_set_evaluation_spectra): [Z][3 E + 1][K][Mv] f64 and the pressure ring [sets Mv][N] f64
    if (s->es_on && is("eval_spectra")) return plain(s->es_tot, 8 * Z * (3 * E + 1) * K * Mv);
    if (s->es_on && is("eval_ring")) return rows_of(StateRef::Ring, s->es_ring, sets * Mv, N, 8);
    // detectability (apv_stream_set_evaluation_detectability): totals [Z][6 E][Mv] f64, [Z][2 E][Mv] per hop of the last call
    if (s->ed_on && is("eval_detect")) return plain(s->ed_tot, 8 * Z * 6 * E * Mv);
    if (s->ed_on && is("eval_detect_hops")) return read_only(plain(s->ed_rec, 8 * Z * 2 * E * Mv * rec));
    // int32 {hops of the last apv_process_signal* call that went through chunk launches, hops of it that went hop by hop}; {0, 0}
    // before the first such call, untouched by the per-hop calls
    if (is("signal_schedule")) return read_only(host(s->sched, sizeof(s->sched)));
    return StateRef();
}

int unknown(apv_handle* h, const char* name) { return apv_fail(h, APV_ERR_STATE, std::string("unknown state name: ") + name); }
int mismatch(apv_handle* h) { return apv_fail(h, APV_ERR_STATE, "state size mismatch"); }
int refuse_set(apv_handle* h, const char* name) { return apv_fail(h, APV_ERR_STATE, std::string(name) + " is read-only"); }

int copy_out(apv_handle* h, void* h_dst, const void* d, size_t bytes) {
    SCHK(h, hipMemcpyAsync(h_dst, d, bytes, hipMemcpyDeviceToHost, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}
int copy_in(apv_handle* h, void* d, const void* h_src, size_t bytes) {
    SCHK(h, hipMemcpyAsync(d, h_src, bytes, hipMemcpyHostToDevice, h->stream));
    SCHK(h, hipStreamSynchronize(h->stream));               // the source may be a temporary of the caller's
    return APV_OK;
}

}  // namespace

extern "C" {

int apv_state_bytes(apv_handle* h, const char* name, size_t* bytes) {
    if (!h || !h->st || !name || !bytes) return apv_fail(h, APV_ERR_ARG, "null argument / no stream");
    const StateRef r = resolve(h, name);
    if (r.kind == StateRef::None) return unknown(h, name);
    *bytes = r.bytes;
    return APV_OK;
}

int apv_get_state(apv_handle* h, const char* name, void* h_dst, size_t bytes) {
    if (!h || !h->st || !name || !h_dst) return apv_fail(h, APV_ERR_ARG, "null argument / no stream");
    apv_stream* s = h->st;
    const StateRef r = resolve(h, name);
    if (r.kind == StateRef::None) return unknown(h, name);
    if (r.kind == StateRef::Live) {
        SCHK(h, hipSetDevice(h->device));
        return apv_live_state(h, s->live, r.index, s->P, s->H, s->C, s->M, s->esz, h_dst, bytes, true, h->stream);
    }
    if (bytes != r.bytes) return mismatch(h);
    if (r.bytes == 0) return APV_OK;                         // "eval_history" with Pv = 1, "eval_hops" before the first hop
    if (r.kind != StateRef::Host || r.settle) SCHK(h, hipSetDevice(h->device));
    if (r.settle) SCHK(h, hipStreamSynchronize(h->stream));
    int rc;
    switch (r.kind) {
    case StateRef::Host:
        std::memcpy(h_dst, r.ptr, r.bytes);
        return APV_OK;
    case StateRef::Plain:
        return copy_out(h, h_dst, r.ptr, r.bytes);
    case StateRef::Ring: {
        std::vector<char> tmp(r.bytes);
        if ((rc = copy_out(h, tmp.data(), r.ptr, r.bytes)) != APV_OK) return rc;
        ring_to_logical(h_dst, tmp.data(), r.rows, r.len, (size_t)s->ring_off, r.esz);
        return APV_OK;
    }
    case StateRef::Grouped: {
        std::vector<char> tmp((size_t)s->Kp * s->C * 2 * s->esz);
        if ((rc = copy_out(h, tmp.data(), r.ptr, tmp.size())) != APV_OK) return rc;
        grouped_to_bin_major(h_dst, tmp.data(), (size_t)s->K, (size_t)s->C, (size_t)s->xg, 2 * s->esz);
        return APV_OK;
    }
    case StateRef::Window:
    case StateRef::Fill: {
        int32_t ctr[2];                                      // {slot the next hop goes to, hops the ring holds}
        if ((rc = copy_out(h, ctr, s->win_ctr, sizeof(ctr))) != APV_OK) return rc;
        if (r.kind == StateRef::Fill) {
            *static_cast<int32_t*>(h_dst) = ctr[1];
            return APV_OK;
        }
        const int T = (int)r.rows, head = ctr[0], fill = ctr[1];
        const size_t slot = r.len * r.esz;
        std::memset(h_dst, 0, r.bytes);
        for (int a = 0; a < fill; ++a) {
            const int from = ((head - fill + a) % T + T) % T;
            SCHK(h, hipMemcpyAsync(static_cast<char*>(h_dst) + (size_t)a * slot, static_cast<char*>(r.ptr) + (size_t)from * slot, slot,
                                   hipMemcpyDeviceToHost, h->stream));
        }
        SCHK(h, hipStreamSynchronize(h->stream));
        return APV_OK;
    }
    default:
        return unknown(h, name);
    }
}

int apv_set_state(apv_handle* h, const char* name, const void* h_src, size_t bytes) {
    if (!h || !h->st || !name || !h_src) return apv_fail(h, APV_ERR_ARG, "null argument / no stream");
    apv_stream* s = h->st;
    const StateRef r = resolve(h, name);
    if (r.kind == StateRef::None || r.get_only) return unknown(h, name);
    if (r.read_only) return refuse_set(h, name);
    if (r.kind == StateRef::Live) {
        SCHK(h, hipSetDevice(h->device));
        SCHK(h, hipStreamSynchronize(h->stream));
        return apv_live_state(h, s->live, r.index, s->P, s->H, s->C, s->M, s->esz, const_cast<void*>(h_src), bytes, false, h->stream);
    }
    if (bytes != r.bytes) return mismatch(h);
    if (r.bytes == 0) return APV_OK;
    SCHK(h, hipSetDevice(h->device));
    if (r.settle) SCHK(h, hipStreamSynchronize(h->stream));
    switch (r.kind) {
    case StateRef::Host:
        return refuse_set(h, name);
    case StateRef::Grouped:
        return apv_fail(h, APV_ERR_STATE, "the control-point spectra are recomputed by every hop and cannot be set");
    case StateRef::Plain:
    case StateRef::Window:                                   // slots in the order of age into slots 0, 1, ...: where a ring stands
        return copy_in(h, r.ptr, h_src, r.bytes);            // does not enter the window sum ("stat_window_fill" says where it goes on)
    case StateRef::Ring: {
        std::vector<char> tmp(r.bytes);
        ring_from_logical(tmp.data(), h_src, r.rows, r.len, (size_t)s->ring_off, r.esz);
        return copy_in(h, r.ptr, tmp.data(), r.bytes);
    }
    case StateRef::Fill: {
        // a restored window lies in slots 0 .. fill - 1: the next hop goes to slot fill mod T
        const int32_t fill = *static_cast<const int32_t*>(h_src), T = s->win_T;
        if (fill < 0 || fill > T) return apv_fail(h, APV_ERR_STATE, "stat_window_fill out of 0..statistics hops");
        const int32_t nw[2] = {fill % T, fill};
        const int rc = copy_in(h, s->win_ctr, nw, sizeof(nw));
        if (rc == APV_OK) s->win_fill_host = fill;
        return rc;
    }
    default:
        return unknown(h, name);
    }
}

}  // extern "C"
