// C ABI of libapvast_hip.so (see include/apvast_hip.h for the contract).
#include "apv_internal.h"
#include "apv_owned.h"
#include <utility>

#include <cmath>
#include <cstdlib>

#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>

namespace {

thread_local std::string g_create_err;
thread_local std::string* g_err_sink = nullptr;      // apv_fail_redirect

int fail(apv_handle* h, int code, const std::string& msg) {
    if (g_err_sink) *g_err_sink = msg;
    else if (h) h->err = msg;
    else g_create_err = msg;
    return code;
}

int hipfail(apv_handle* h, hipError_t e, const char* what) {
    return fail(h, APV_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIPCHK(h, call)                                   \
    do {                                                  \
        hipError_t _e = (call);                           \
        if (_e != hipSuccess) return hipfail(h, _e, #call); \
    } while (0)

size_t csize(const apv_handle* h) { return h->cfg.compute_dtype == APV_F64 ? 16 : 8; }
size_t wsize(const apv_handle* h) { return h->cfg.out_c128 ? 16 : 8; }
size_t lsize(const apv_handle* h) { return h->cfg.out_c128 ? 8 : 4; }

}  // namespace

int apv_fail(apv_handle* h, int code, const std::string& msg) { return fail(h, code, msg); }
void apv_fail_redirect(std::string* sink) { g_err_sink = sink; }

GevdParams apv_base_params(const apv_handle* h);

namespace {

GevdParams base_params(const apv_handle* h) { return apv_base_params(h); }

}  // namespace

GevdParams apv_base_params(const apv_handle* h) {
    GevdParams p;
    std::memset(&p, 0, sizeof(p));
    const apv_config& c = h->cfg;
    p.n = c.n_srcs;
    p.M = c.n_mics;
    p.K = c.n_bins;
    p.nV = c.n_ranks;
    // (lists longer than APV_MAX_RANKS -- orders above 64 only -- reach kernels_gevd128.hip through apv_launch_gevd's ranks_all)
    const int nr = c.n_ranks < APV_MAX_RANKS ? c.n_ranks : APV_MAX_RANKS;
    for (int i = 0; i < nr; ++i) p.ranks[i] = h->rank_list.empty() ? c.ranks[i] : h->rank_list[i];
    p.mu = c.mu;
    p.reg_dark = c.reg_dark;
    p.reg_bright = c.reg_bright;
    p.reg_mode = c.reg_mode;
    p.max_sweeps = c.max_sweeps;
    p.debug_stop = c.debug_stop;
    p.sweep_tol2 = c.sweep_tol2;
    p.out_c128 = c.out_c128;
    p.Lspill = h->d_Lspill;
    p.stamps = h->d_stamps;
    // the span of the handle (apv_set_span): row z of its tables and outputs for zone program z
    const apv_handle::Span& sp = h->span;
    if (sp.on) {
        const size_t K = c.n_bins, L = c.n_srcs;
        p.span.on = 1;
        p.span.phi = sp.phi;
        for (size_t z = 0; z < 2; ++z) {
            p.span.z[z].mu_eff = sp.d_mu_eff ? sp.d_mu_eff + z * K : nullptr;
            p.span.z[z].cap = sp.d_cap ? sp.d_cap + z * K : nullptr;
            p.span.z[z].rank = sp.d_rank + z * K;
            p.span.z[z].contrast = sp.d_contrast ? sp.d_contrast + z * K * L : nullptr;
        }
    }
    return p;
}

namespace {

int ensure_spill(apv_handle* h, int n, int K) {
    const apv_config& c = h->cfg;
    const size_t need = apv_gevd_spill_bytes(n, K, c.compute_dtype, c.reg_mode, c.reg_bright, c.sweep_tol2, c.n_zones == 3 ? 2 : 1);
    if (need > h->lspill_bytes) {
        if (h->d_Lspill) HIPCHK(h, hipFree(h->d_Lspill));
        h->d_Lspill = nullptr;
        h->lspill_bytes = 0;
        if (h->d_Lspill_lane1) {          // (too small now: launches that need the scratch keep to one lane until pipelining is set again)
            HIPCHK(h, hipFree(h->d_Lspill_lane1));
            h->d_Lspill_lane1 = nullptr;
        }
        HIPCHK(h, hipMalloc(&h->d_Lspill, need));
        h->lspill_bytes = need;
    }
    return APV_OK;
}

// scratch R of the split float32 update at orders 32 / 64 (apv_update_dev): correlation on the f32 matrix cores -> [2][K][L][L] +
// [K][L] c64 -> LDS kernel.  Sized at apv_create so that the per-block path never allocates.
bool split_f32_update(const apv_config& c) {
    const bool split64 = c.n_srcs == 64 && !apv_gevd64_eligible(c.n_srcs, c.reg_mode, c.reg_bright, c.sweep_tol2);
    return c.compute_dtype == APV_F32 && (c.n_srcs == 32 || split64) && (c.n_mics % 2) == 0 && c.n_mics >= 8;
}

int ensure_rscratch(apv_handle* h) {
    const apv_config& c = h->cfg;
    if (!split_f32_update(c)) return APV_OK;
    const size_t K = c.n_bins, L = c.n_srcs;
    const size_t need = (2 * K * L * L + K * L) * 8;
    if (need > h->rscratch_bytes) {
        if (h->d_Rscratch) HIPCHK(h, hipFree(h->d_Rscratch));
        h->d_Rscratch = nullptr;
        h->rscratch_bytes = 0;
        HIPCHK(h, hipMalloc(&h->d_Rscratch, need ? need : 1));
        h->rscratch_bytes = need;
    }
    return APV_OK;
}

int ensure_staging(apv_handle* h) {
    if (h->d_XB) return APV_OK;
    const apv_config& c = h->cfg;
    const size_t K = c.n_bins, M = c.n_mics, L = c.n_srcs;
    HIPCHK(h, hipMalloc(&h->d_XB, K * M * L * 8));
    HIPCHK(h, hipMalloc(&h->d_XD, K * M * L * 8));
    HIPCHK(h, hipMalloc(&h->d_d, K * M * 8));
    HIPCHK(h, hipMalloc(&h->d_w, K * c.n_ranks * L * 16));
    HIPCHK(h, hipMalloc(&h->d_lam, K * L * 8));
    HIPCHK(h, hipMalloc((void**)&h->d_status, K * sizeof(int32_t)));
    return APV_OK;
}


// ---- update lanes (apv_set_update_streams) -----------------------------------------------------------------------------------
// With two lanes (the handle's stream and one more), launch i + 1 of apv_update_dev starts on the other lane while the waves of launch i's last round are still
// finishing (a cfg2 launch is 8 rounds of 4 waves per SIMD; 3.6 of 4 alive on average: profiles/r03/stage_stamps_32768_b.md).
// Ordering is by events, never by the host:
//   lanes_join   the control stream waits for the latest launch of every lane (before anything it is asked to do with buffers)
//   lanes_fork   a lane waits for what the control stream has been given since the lanes last looked (ctrl_dirty)
//   operand ranges of the latest launch of the OTHER lane: a launch that writes what it reads or writes, or reads what it writes, waits
//   for it; and every launch waits for the other lane's launch BEFORE its latest, so that the latest is the only launch of the other
//   lane it can ever run beside (the ranges of one launch per lane are then all there is to compare; in the steady state that
//   event completed a launch ago)
bool lanes_on(const apv_handle* h) { return h->n_lanes > 1; }

int lanes_join(apv_handle* h, bool dirties) {
    if (!lanes_on(h)) return APV_OK;
    for (auto& ln : h->lane)
        if (ln.used) HIPCHK(h, hipStreamWaitEvent(h->stream, ln.ev, 0));
    if (dirties) h->ctrl_dirty = true;
    return APV_OK;
}

bool ranges_meet(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

int lanes_sync(apv_handle* h) {
    for (auto& ln : h->lane)
        if (ln.s) HIPCHK(h, hipStreamSynchronize(ln.s));
    return APV_OK;
}

}  // namespace

// The blocks apv_host_alloc has handed out (page-locked, visible to every device): a result pointer inside one of them takes a
// device-to-host copy by DMA.  A table of our own, because asking the runtime about an arbitrary pointer
// (hipPointerGetAttributes) costs a search and, for pageable memory, an error path on every call.
namespace {
std::mutex g_host_blocks_mu;
std::map<uintptr_t, size_t> g_host_blocks;
}  // namespace

void apv_host_blocks_note(const void* p, size_t bytes, bool add) {
    std::lock_guard<std::mutex> lk(g_host_blocks_mu);
    if (add) g_host_blocks[(uintptr_t)p] = bytes;
    else g_host_blocks.erase((uintptr_t)p);
}

bool apv_host_block_contains(const void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_host_blocks_mu);
    auto it = g_host_blocks.upper_bound((uintptr_t)p);
    if (it == g_host_blocks.begin()) return false;
    --it;
    return (uintptr_t)p >= it->first && (uintptr_t)p + bytes <= it->first + it->second;
}

extern "C" {

int apv_abi_version(void) { return APV_ABI_VERSION; }

const char* apv_last_error(const apv_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int apv_create(const apv_config* cfg, apv_handle** out) {
    if (!cfg || !out) return fail(nullptr, APV_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->abi_version != APV_ABI_VERSION) return fail(nullptr, APV_ERR_ARG, "ABI version mismatch");
    if (cfg->n_srcs < 1 || cfg->n_srcs > APV_MAX_SRCS) return fail(nullptr, APV_ERR_ARG, "n_srcs must be in 1..128");
    if (cfg->n_bins < 0 || cfg->n_mics < 1) return fail(nullptr, APV_ERR_ARG, "n_bins/n_mics out of range");
    if (cfg->n_ranks < 1 || cfg->n_ranks > APV_MAX_RANKS) return fail(nullptr, APV_ERR_ARG, "n_ranks must be in 1..64");
    for (int i = 0; i < cfg->n_ranks; ++i) {
        if (cfg->ranks[i] < 1 || cfg->ranks[i] > cfg->n_srcs) return fail(nullptr, APV_ERR_ARG, "rank V out of 1..L");
        if (i && cfg->ranks[i] <= cfg->ranks[i - 1]) return fail(nullptr, APV_ERR_ARG, "ranks must be ascending");
    }
    if (cfg->compute_dtype != APV_F32 && cfg->compute_dtype != APV_F64)
        return fail(nullptr, APV_ERR_ARG, "compute_dtype must be APV_F32 or APV_F64");
    if (cfg->reg_mode != APV_REG_ABS && cfg->reg_mode != APV_REG_REL)
        return fail(nullptr, APV_ERR_ARG, "reg_mode must be APV_REG_ABS or APV_REG_REL");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return fail(nullptr, APV_ERR_HIP, "no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, APV_ERR_ARG, "device ordinal out of range");
    apv_handle* h = new (std::nothrow) apv_handle();
    if (!h) return fail(nullptr, APV_ERR_HIP, "out of host memory");
    h->cfg = *cfg;
    h->rank_list.assign(cfg->ranks, cfg->ranks + cfg->n_ranks);
    h->device = cfg->device;
    h->stream = nullptr;
    h->ev0 = h->ev1 = nullptr;
    h->d_XB = h->d_XD = h->d_d = h->d_w = h->d_lam = nullptr;
    h->d_status = nullptr;
    h->d_Lspill = nullptr;
    h->lspill_bytes = 0;
    h->d_Rscratch = nullptr;
    h->rscratch_bytes = 0;
    h->d_stamps = nullptr;
    h->st = nullptr;
    h->bb = nullptr;
    h->stat_hops = 1;
    h->stat_forgetting = 0.0;
    h->filter_taps = 0;
    h->synthesis = APV_SYNTH_WOLA;
    h->eval_Pv = h->eval_Mv = 0;
    h->eval_spectra = 0;
    h->eval_detect_C = 0;
    h->eval_detect_Cs = h->eval_detect_Ca = h->eval_detect_Leff = 0.0;
    h->gl_ws = nullptr;
    h->gl_tol2 = 0.0;
    h->gl_lead_rank = 0;
    h->gl_lead_done = 0;
    h->lead_ws = nullptr;
    h->comm_stream = nullptr;
    h->ev_ready = nullptr;
    for (auto& g : h->gather_done) { g.ptr = nullptr; g.ev = nullptr; }
    h->gather_next = 0;
    h->ev_ag0 = h->ev_ag1 = nullptr;
    h->ag_bytes = 0;
    h->d_bar = nullptr;
    h->comm = nullptr;
    h->comm_rank = 0;
    h->comm_world = 1;
    for (auto& ln : h->lane) {
        ln.s = nullptr;
        ln.ev = ln.ev_prev = nullptr;
        ln.used = ln.used_prev = ln.need_fork = false;
        for (int i = 0; i < 3; ++i) { ln.rd[i] = ln.wr[i] = nullptr; ln.rd_bytes[i] = ln.wr_bytes[i] = 0; }
    }
    h->d_Lspill_lane1 = nullptr;
    h->n_lanes = 1;
    h->lane_next = 0;
    h->ctrl_dirty = false;
    h->ev_fork = nullptr;
#define CR(call)                                                         \
    do {                                                                 \
        hipError_t _e = (call);                                          \
        if (_e != hipSuccess) {                                          \
            g_create_err = std::string(#call) + ": " + hipGetErrorString(_e); \
            apv_destroy(h);                                              \
            return APV_ERR_HIP;                                          \
        }                                                                \
    } while (0)
    CR(hipSetDevice(h->device));
    CR(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CR(hipEventCreate(&h->ev0));
    CR(hipEventCreate(&h->ev1));
#undef CR
    int rc = ensure_spill(h, cfg->n_srcs, cfg->n_bins);
    if (rc == APV_OK) rc = ensure_rscratch(h);
    if (rc != APV_OK) {
        g_create_err = h->err;
        apv_destroy(h);
        return rc;
    }
    *out = h;
    return APV_OK;
}

int apv_destroy(apv_handle* h) {
    if (!h) return APV_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    apv_stream_free(h);
    apv_bb_free(h);
    apv_gevd_large_free(h);
    apv_gevd_lead_free(h);
    if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
    for (auto& ln : h->lane) {
        if (ln.s) (void)hipStreamSynchronize(ln.s);
        if (ln.ev) (void)hipEventDestroy(ln.ev);
        if (ln.ev_prev) (void)hipEventDestroy(ln.ev_prev);
        if (ln.s && ln.s != h->stream) (void)hipStreamDestroy(ln.s);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->comm) ncclCommDestroy((ncclComm_t)h->comm);
    for (auto& g : h->gather_done)
        if (g.ev) (void)hipEventDestroy(g.ev);
    if (h->ev_ready) (void)hipEventDestroy(h->ev_ready);
    if (h->ev_ag0) (void)hipEventDestroy(h->ev_ag0);
    if (h->ev_ag1) (void)hipEventDestroy(h->ev_ag1);
    if (h->d_bar) (void)hipFree(h->d_bar);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    void* bufs[] = {h->d_XB, h->d_XD, h->d_d, h->d_w, h->d_lam, h->d_status, h->d_Lspill, h->d_Lspill_lane1, h->d_Rscratch,
                    h->span.d_mu_eff, h->span.d_cap, h->span.d_rank, h->span.d_contrast};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    delete h->effort.own;
    delete h->valspan.own;
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return APV_OK;
}

int apv_dev_alloc(apv_handle* h, size_t bytes, void** d_ptr) {
    if (!h || !d_ptr) return APV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMalloc(d_ptr, bytes ? bytes : 1));
    return APV_OK;
}

int apv_dev_free(apv_handle* h, void* d_ptr) {
    if (!h) return APV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipFree(d_ptr));
    return APV_OK;
}

int apv_memcpy_h2d(apv_handle* h, void* d_dst, const void* h_src, size_t bytes) {
    if (!h) return APV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;          // a launch in flight may still read what this copy overwrites
    HIPCHK(h, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, h->stream));
    return APV_OK;
}

int apv_memcpy_d2h(apv_handle* h, void* h_dst, const void* d_src, size_t bytes) {
    if (!h) return APV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;          // (dirty: a later launch must not overwrite the source under the copy)
    HIPCHK(h, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, h->stream));
    return APV_OK;
}

int apv_sync(apv_handle* h) {
    if (!h) return APV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_sync(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
    return APV_OK;
}

int apv_timer_start(apv_handle* h) {
    if (!h) return APV_ERR_ARG;
    if (int rc = lanes_join(h, false)) return rc;
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    return APV_OK;
}

int apv_timer_stop(apv_handle* h, float* elapsed_ms) {
    if (!h || !elapsed_ms) return APV_ERR_ARG;
    if (int rc = lanes_join(h, false)) return rc;          // the interval ends behind the latest launch of every lane
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return APV_OK;
}

int apv_update_dev(apv_handle* h, const void* d_XB, const void* d_XD, const void* d_d, void* d_w, void* d_lam,
                   int32_t* d_status) {
    if (!h) return APV_ERR_ARG;
    if (h->cfg.n_bins == 0) return APV_OK;
    if (!d_XB || !d_XD || !d_d || !d_w) return fail(h, APV_ERR_ARG, "null device pointer");
    HIPCHK(h, hipSetDevice(h->device));
    const apv_config& c = h->cfg;
    // the stream of this launch: the handle's own, or (apv_set_update_streams) the next lane.  Orders 33..64 park per-bin state in
    // scratch slots: lane 1 has slots of its own (d_Lspill_lane1).  The split float32 update shares ONE scratch R: its launches
    // all take lane 0, one after the other.
    hipStream_t st = h->stream;
    apv_handle::UpdateLane* ln = nullptr;
    if (lanes_on(h)) {
        const bool shares_scratch = (h->d_Lspill != nullptr && h->d_Lspill_lane1 == nullptr) || split_f32_update(c);
        const int li = shares_scratch ? 0 : h->lane_next;
        if (!shares_scratch) h->lane_next ^= 1;
        ln = &h->lane[li];
        st = ln->s;
        if (h->ctrl_dirty) {              // copies (or other work) went to the control stream since the lanes last looked
            HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
            for (auto& l2 : h->lane) l2.need_fork = true;
            h->ctrl_dirty = false;
        }
        if (ln->need_fork) {
            HIPCHK(h, hipStreamWaitEvent(st, h->ev_fork, 0));
            ln->need_fork = false;
        }
        const size_t K = c.n_bins, M = c.n_mics, L = c.n_srcs;
        const void* rd[3] = {d_XB, d_XD, d_d};
        const size_t rd_bytes[3] = {K * M * L * 8, K * M * L * 8, K * M * 8};
        const void* wr[3] = {d_w, d_lam, d_status};
        const size_t wr_bytes[3] = {K * c.n_ranks * L * wsize(h), d_lam ? K * L * lsize(h) : 0, d_status ? K * sizeof(int32_t) : 0};
        apv_handle::UpdateLane& other = h->lane[li ^ 1];
        if (other.used_prev) HIPCHK(h, hipStreamWaitEvent(st, other.ev_prev, 0));
        if (other.used) {
            bool clash = false;
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j)
                    clash = clash || ranges_meet(wr[i], wr_bytes[i], other.wr[j], other.wr_bytes[j]) ||
                            ranges_meet(wr[i], wr_bytes[i], other.rd[j], other.rd_bytes[j]) ||
                            ranges_meet(rd[i], rd_bytes[i], other.wr[j], other.wr_bytes[j]);
            if (clash) HIPCHK(h, hipStreamWaitEvent(st, other.ev, 0));
        }
        for (int i = 0; i < 3; ++i) {
            ln->rd[i] = rd[i]; ln->rd_bytes[i] = rd_bytes[i];
            ln->wr[i] = wr[i]; ln->wr_bytes[i] = wr_bytes[i];
        }
    }
    for (auto& g : h->gather_done)
        if (g.ptr == d_w && g.ev) {       // an all-gather may still be reading this shard buffer
            HIPCHK(h, hipStreamWaitEvent(st, g.ev, 0));
            g.ptr = nullptr;
        }
    GevdParams p = base_params(h);
    if (ln == &h->lane[1] && h->d_Lspill_lane1) p.Lspill = h->d_Lspill_lane1;
    p.w = d_w;
    p.lam = d_lam;
    p.status = d_status;
    // slabs of rank below the order: not for kernels_gevd64.hip (apv_internal.h).  A float32 handle keeps that kernel and its
    // float64 fall-back: the float LDS kernel it would get instead is the less accurate of the two
    p.no_gevd64 = c.n_mics < c.n_srcs && c.compute_dtype == APV_F64;
    std::string why;
    hipError_t e;
    // order 64 takes the fused order-64 kernel in either arithmetic (kernels_gevd64.hip) unless that kernel is switched off
    if (split_f32_update(c)) {
        // large orders in f32: correlation on the f32 matrix cores into a scratch R (HBM round trip of
        // 2 L^2 c64 per bin, small against the eigen-iteration), then the LDS-resident GEVD from explicit R.  The scratch was
        // sized by apv_create (ensure_rscratch): nothing is allocated here.
        const size_t K = c.n_bins, L = c.n_srcs;
        if (!h->d_Rscratch || (2 * K * L * L + K * L) * 8 > h->rscratch_bytes) return fail(h, APV_ERR_STATE, "scratch R missing");
        float2* RB = (float2*)h->d_Rscratch;
        float2* RD = RB + K * L * L;
        float2* rr = RD + K * L * L;
        e = apv_launch_corr(APV_F32, c.n_bins, c.n_mics, c.n_srcs, (const float2*)d_XB, (const float2*)d_XD,
                            (const float2*)d_d, RB, RD, rr, st);
        if (e != hipSuccess) return hipfail(h, e, "corr launch");
        p.RB = RB;
        p.RD = RD;
        p.r = rr;
        e = apv_launch_gevd(p, APV_F32, false, st, &why);
    } else {
        p.XB = (const float2*)d_XB;
        p.XD = (const float2*)d_XD;
        p.d = (const float2*)d_d;
        e = apv_launch_gevd(p, h->cfg.compute_dtype, true, st, &why, h->rank_list.data());
    }
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    if (ln) {
        std::swap(ln->ev, ln->ev_prev);              // the latest becomes the one before; its handle is recorded anew
        ln->used_prev = ln->used;
        HIPCHK(h, hipEventRecord(ln->ev, st));
        ln->used = true;
    }
    return APV_OK;
}

int apv_set_update_streams(apv_handle* h, int32_t n) {
    if (!h) return APV_ERR_ARG;
    if (n != 1 && n != 2) return fail(h, APV_ERR_ARG, "update streams: 1 or 2");
    if (n == 2 && h->span.on) return fail(h, APV_ERR_ARG, "update streams: one with a span (its outputs are one buffer)");
    HIPCHK(h, hipSetDevice(h->device));
    // drain first: whatever is in flight was ordered under the old scheme
    if (int rc = lanes_sync(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n == 2 && !h->lane[0].s) {
        // Lane 0 IS the handle's control stream, lane 1 a stream of its own: the runtime deals a process's streams over four hardware
        // queues and every stream fewer is one fewer to share them with (with the gather's stream the sharded path then has three
        // streams and the lanes work beside the collective; with a control stream of its own they did not: DESIGN.md 4.9).  Waiting for
        // its own events costs the control stream nothing; a join (copies, timers) holds back lane 0's NEXT launch until lane 1's
        // latest has ended -- once per copy, not per launch.
        for (auto& ln : h->lane) {
            if (&ln == &h->lane[0]) ln.s = h->stream;
            else HIPCHK(h, hipStreamCreateWithFlags(&ln.s, hipStreamNonBlocking));
            HIPCHK(h, hipEventCreateWithFlags(&ln.ev, hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&ln.ev_prev, hipEventDisableTiming));
        }
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    }
    if (n == 2 && h->lspill_bytes > 0 && !h->d_Lspill_lane1) HIPCHK(h, hipMalloc(&h->d_Lspill_lane1, h->lspill_bytes));
    for (auto& ln : h->lane) ln.used = ln.used_prev = ln.need_fork = false;
    h->ctrl_dirty = false;
    h->lane_next = 0;
    h->n_lanes = n;
    return APV_OK;
}

static int scan_status(apv_handle* h, const int32_t* st, int K) {
    int rc = APV_OK;
    for (int k = 0; k < K; ++k) {
        if (st[k] == 1) {
            char buf[96];
            std::snprintf(buf, sizeof(buf), "Matrix is not positive definite (bin %d)", k);
            return fail(h, APV_ERR_NOT_PD, buf);
        }
        if (st[k] == 2 && rc == APV_OK) {
            char buf[96];
            std::snprintf(buf, sizeof(buf), "eigen-iteration did not converge (bin %d)", k);
            h->err = buf;
            rc = APV_ERR_NO_CONVERGE;
        }
    }
    return rc;
}

int apv_update(apv_handle* h, const float* h_XB, const float* h_XD, const float* h_d, void* h_w, void* h_lam,
               int32_t* h_status) {
    if (!h) return APV_ERR_ARG;
    if (h->cfg.n_bins == 0) return APV_OK;
    if (!h_XB || !h_XD || !h_d || !h_w) return fail(h, APV_ERR_ARG, "null host pointer");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ensure_staging(h);
    if (rc != APV_OK) return rc;
    const apv_config& c = h->cfg;
    const size_t K = c.n_bins, M = c.n_mics, L = c.n_srcs;
    if ((rc = lanes_join(h, true)) != APV_OK) return rc;          // the staging buffers may still be read by a launch in flight
    HIPCHK(h, hipMemcpyAsync(h->d_XB, h_XB, K * M * L * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_XD, h_XD, K * M * L * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_d, h_d, K * M * 8, hipMemcpyHostToDevice, h->stream));
    rc = apv_update_dev(h, h->d_XB, h->d_XD, h->d_d, h->d_w, h->d_lam, h->d_status);
    if (rc != APV_OK) return rc;
    if ((rc = lanes_join(h, true)) != APV_OK) return rc;
    HIPCHK(h, hipMemcpyAsync(h_w, h->d_w, K * c.n_ranks * L * wsize(h), hipMemcpyDeviceToHost, h->stream));
    if (h_lam) HIPCHK(h, hipMemcpyAsync(h_lam, h->d_lam, K * L * lsize(h), hipMemcpyDeviceToHost, h->stream));
    std::string keep;
    int32_t* st = h_status;
    std::unique_ptr<int32_t[]> tmp;
    if (!st) {
        tmp.reset(new int32_t[K ? K : 1]);
        st = tmp.get();
    }
    HIPCHK(h, hipMemcpyAsync(st, h->d_status, K * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return scan_status(h, st, (int)K);
}

int apv_corr_dev(apv_handle* h, const void* d_XB, const void* d_XD, const void* d_d, void* d_RB, void* d_RD,
                 void* d_r) {
    if (!h || !d_XB || !d_XD || !d_d || !d_RB || !d_RD || !d_r) return fail(h, APV_ERR_ARG, "null device pointer");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    const apv_config& c = h->cfg;
    // (a handle may have up to 128 loudspeakers; the kernels behind this entry point hold an order of at most APV_MAX_N)
    if (c.n_srcs > APV_MAX_N) return fail(h, APV_ERR_ARG, "apv_corr_dev: n_srcs must be in 1..64");
    hipError_t e = apv_launch_corr(c.compute_dtype, c.n_bins, c.n_mics, c.n_srcs, (const float2*)d_XB,
                                   (const float2*)d_XD, (const float2*)d_d, d_RB, d_RD, d_r, h->stream);
    if (e != hipSuccess) return hipfail(h, e, "corr launch");
    return APV_OK;
}

int apv_to_bf16_dev(apv_handle* h, size_t count, const void* d_c64, void* d_bf16) {
    if (!h || !d_c64 || !d_bf16) return fail(h, APV_ERR_ARG, "null device pointer");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    hipError_t e = apv_launch_to_bf16(count, (const float2*)d_c64, (uint32_t*)d_bf16, h->stream);
    if (e != hipSuccess) return hipfail(h, e, "to_bf16 launch");
    return APV_OK;
}

int apv_corr_bf16_dev(apv_handle* h, const void* d_XB, const void* d_XD, const void* d_d, void* d_RB, void* d_RD,
                      void* d_r) {
    if (!h || !d_XB || !d_XD || !d_d || !d_RB || !d_RD || !d_r) return fail(h, APV_ERR_ARG, "null device pointer");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    const apv_config& c = h->cfg;
    if ((c.n_srcs != 32 && c.n_srcs != 64) || (c.n_mics % 16) != 0)
        return fail(h, APV_ERR_ARG, "bf16 correlation: n_srcs must be 32 or 64 and n_mics a multiple of 16");
    hipError_t e = apv_launch_corr_bf16(c.n_bins, c.n_mics, c.n_srcs, (const uint32_t*)d_XB, (const uint32_t*)d_XD,
                                        (const uint32_t*)d_d, (float2*)d_RB, (float2*)d_RD, (float2*)d_r, h->stream);
    if (e != hipSuccess) return hipfail(h, e, "corr_bf16 launch");
    return APV_OK;
}

int apv_gevd_vast_dev(apv_handle* h, const void* d_RB, const void* d_RD, const void* d_r, void* d_w, void* d_lam,
                      int32_t* d_status) {
    if (!h || !d_RB || !d_RD || !d_r || !d_w) return fail(h, APV_ERR_ARG, "null device pointer");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    GevdParams p = base_params(h);
    p.RB = d_RB;
    p.RD = d_RD;
    p.r = d_r;
    p.w = d_w;
    p.lam = d_lam;
    p.status = d_status;
    std::string why;
    hipError_t e = apv_launch_gevd(p, h->cfg.compute_dtype, false, h->stream, &why, h->rank_list.data());
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_set_rank_list(apv_handle* h, int32_t n, const int32_t* ranks) {
    if (!h) return APV_ERR_ARG;
    if (h->st) return fail(h, APV_ERR_STATE, "apv_set_rank_list: the stream is initialised (its buffers are sized by the rank count)");
    const int L = h->cfg.n_srcs;
    if (n < 1 || n > L || !ranks) return fail(h, APV_ERR_ARG, "rank list: between 1 and n_srcs ranks");
    for (int i = 0; i < n; ++i) {
        if (ranks[i] < 1 || ranks[i] > L) return fail(h, APV_ERR_ARG, "rank V out of 1..L");
        if (i && ranks[i] <= ranks[i - 1]) return fail(h, APV_ERR_ARG, "ranks must be ascending");
    }
    if (n > APV_MAX_RANKS && L <= APV_MAX_N) return fail(h, APV_ERR_ARG, "more than 64 ranks need n_srcs > 64");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_sync(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the host-buffer staging is sized by the rank count: reallocated at the next apv_update
    void** bufs[] = {&h->d_XB, &h->d_XD, &h->d_d, &h->d_w, &h->d_lam, reinterpret_cast<void**>(&h->d_status)};
    for (void** b : bufs) {
        if (*b) HIPCHK(h, hipFree(*b));
        *b = nullptr;
    }
    h->rank_list.assign(ranks, ranks + n);
    h->cfg.n_ranks = n;
    const int head = n < APV_MAX_RANKS ? n : APV_MAX_RANKS;
    for (int i = 0; i < APV_MAX_RANKS; ++i) h->cfg.ranks[i] = i < head ? ranks[i] : 0;
    return APV_OK;
}

int apv_jdiag_batched(apv_handle* h, int32_t n, int32_t batch, const double* h_A, const double* h_B, double* h_U,
                      double* h_lam, int32_t* h_status) {
    if (!h || !h_A || !h_B || !h_U || !h_lam) return fail(h, APV_ERR_ARG, "null host pointer");
    if (n < 1 || n > APV_MAX_N || batch < 0) return fail(h, APV_ERR_ARG, "jdiag order n must be in 1..64");
    if (batch == 0) return APV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // always runs in f64 / c128, whatever the handle's streaming dtype
    const size_t mat = (size_t)batch * n * n * 16;
    ApvOwned t;                                             // freed on every way out
    void *dA = nullptr, *dB = nullptr, *dU = nullptr, *dw = nullptr, *dl = nullptr, *spill = nullptr;
    int32_t* ds = nullptr;
    HIPCHK(h, t.device(&dA, mat));
    HIPCHK(h, t.device(&dB, mat));
    HIPCHK(h, t.device(&dU, mat));
    HIPCHK(h, t.device(&dw, (size_t)batch * n * 16));
    HIPCHK(h, t.device(&dl, (size_t)batch * n * 8));
    HIPCHK(h, t.device(&ds, (size_t)batch * sizeof(int32_t)));
    const size_t sb = apv_gevd_spill_bytes(n, batch, APV_F64, h->cfg.reg_mode, 0.0, 1e-17, 1);   // as launched below: f64, tol 1e-17
    if (sb) HIPCHK(h, t.device(&spill, sb));
    HIPCHK(h, hipMemcpyAsync(dA, h_A, mat, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dB, h_B, mat, hipMemcpyHostToDevice, h->stream));
    GevdParams p = base_params(h);
    p.span = SpanParams{};         // another order and batch than the span's tables; U and lambda do not depend on it
    p.n = n;
    p.K = batch;
    p.nV = 1;
    p.ranks[0] = 1;
    p.reg_bright = 0.0;
    p.sweep_tol2 = 1e-17;          // drop-in for jdiag: iterate to working precision
    p.out_c128 = 1;
    p.RB = dA;
    p.RD = dB;
    p.r = nullptr;
    p.w = dw;
    p.lam = dl;
    p.status = ds;
    p.U = dU;
    p.Lspill = spill;
    std::string why;
    hipError_t e = apv_launch_gevd(p, APV_F64, false, h->stream, &why);
    int rc = APV_OK;
    if (e != hipSuccess) rc = fail(h, APV_ERR_HIP, why.empty() ? hipGetErrorString(e) : why);
    std::unique_ptr<int32_t[]> tmp;
    int32_t* st = h_status;
    if (!st) {
        tmp.reset(new int32_t[batch]);
        st = tmp.get();
    }
    if (rc == APV_OK) {
        (void)hipMemcpyAsync(h_U, dU, mat, hipMemcpyDeviceToHost, h->stream);
        (void)hipMemcpyAsync(h_lam, dl, (size_t)batch * n * 8, hipMemcpyDeviceToHost, h->stream);
        (void)hipMemcpyAsync(st, ds, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream);
        hipError_t se = hipStreamSynchronize(h->stream);
        if (se != hipSuccess) rc = hipfail(h, se, "jdiag sync");
    }
    if (rc != APV_OK) return rc;
    return scan_status(h, st, batch);
}

int apv_jdiag_large(apv_handle* h, int32_t n, int32_t batch, const double* h_A, const double* h_B, double* h_U,
                    double* h_lam, int32_t* h_status) {
    if (!h || !h_A || !h_B || !h_U || !h_lam) return fail(h, APV_ERR_ARG, "null host pointer");
    if (n < 1 || n > 4096 || batch < 0) return fail(h, APV_ERR_ARG, "apv_jdiag_large: n must be in 1..4096");
    if (batch == 0) return APV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t mat = (size_t)batch * n * n * sizeof(double);
    ApvOwned t;                                             // freed on every way out
    double *dA = nullptr, *dB = nullptr, *dU = nullptr, *dl = nullptr, *dn = nullptr;
    HIPCHK(h, t.device(&dA, mat));
    HIPCHK(h, t.device(&dB, mat));
    HIPCHK(h, t.device(&dU, mat));
    HIPCHK(h, t.device(&dl, (size_t)batch * n * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(dA, h_A, mat, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dB, h_B, mat, hipMemcpyHostToDevice, h->stream));
    std::unique_ptr<int32_t[]> tmp;
    int32_t* st = h_status;
    if (!st) {
        tmp.reset(new int32_t[batch]);
        st = tmp.get();
    }
    if (h->cfg.reg_mode == APV_REG_REL) {
        // B + reg_dark ||B||_2 I (apvast.py:26-27): the spectral norms first, four matrices per launch
        HIPCHK(h, t.device(&dn, (size_t)batch * sizeof(double)));
        for (int z0 = 0; z0 < batch; z0 += 4) {
            const double* mats[4];
            const int cnt = batch - z0 < 4 ? batch - z0 : 4;
            for (int q = 0; q < cnt; ++q) mats[q] = dB + (size_t)(z0 + q) * n * n;
            HIPCHK(h, apv_launch_norm2(n, cnt, mats, dn + z0, h->stream));
        }
    }
    int rc = apv_gevd_large(h, n, batch, dA, dB, h->cfg.reg_dark, dn, dU, dl, nullptr, 0.0, 0, nullptr, nullptr, st);
    if (rc == APV_OK || rc == APV_ERR_NOT_PD) {
        (void)hipMemcpyAsync(h_U, dU, mat, hipMemcpyDeviceToHost, h->stream);
        (void)hipMemcpyAsync(h_lam, dl, (size_t)batch * n * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        (void)hipStreamSynchronize(h->stream);
    }
    if (rc != APV_OK) return rc;
    for (int z = 0; z < batch; ++z)
        if (st[z] == 2) return fail(h, APV_ERR_NO_CONVERGE, "eigen-iteration did not converge");
    return APV_OK;
}

int apv_norm2(apv_handle* h, int32_t n, int32_t count, const double* h_mats, double* h_out, int32_t method) {
    if (!h || !h_mats || !h_out) return fail(h, APV_ERR_ARG, "null host pointer");
    if (n < 1 || n > APV_NORM2_MAX_N || count < 0) return fail(h, APV_ERR_ARG, "apv_norm2: n must be in 1..4096");
    if (method != APV_NORM2_AUTO && method != APV_NORM2_ONE_WG && method != APV_NORM2_GRID)
        return fail(h, APV_ERR_ARG, "apv_norm2: unknown method");
    if (count == 0) return APV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t nn = (size_t)n * n;
    ApvOwned t;                                             // buffers and timing events: freed on every way out
    double *dM = nullptr, *dn = nullptr;
    HIPCHK(h, t.device(&dM, sizeof(double) * nn * count));
    HIPCHK(h, t.device(&dn, sizeof(double) * count));
    HIPCHK(h, hipMemcpyAsync(dM, h_mats, sizeof(double) * nn * count, hipMemcpyHostToDevice, h->stream));
    // APV_BB_TIMING=1: the device time of the norms alone, between two events (profiling aid, as in stream_bb.hip)
    static const bool timing = getenv("APV_BB_TIMING") != nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (timing) {
        HIPCHK(h, t.event(&ev[0], hipEventDefault));
        HIPCHK(h, t.event(&ev[1], hipEventDefault));
        HIPCHK(h, hipEventRecord(ev[0], h->stream));
    }
    for (int z0 = 0; z0 < count; z0 += 4) {          // four matrices per call, as a hop has them
        const double* mats[4];
        const int cnt = count - z0 < 4 ? count - z0 : 4;
        for (int q = 0; q < cnt; ++q) mats[q] = dM + (size_t)(z0 + q) * nn;
        HIPCHK(h, apv_launch_norm2(n, cnt, mats, dn + z0, h->stream, method));
    }
    if (timing) {
        float ms = 0.0f;
        HIPCHK(h, hipEventRecord(ev[1], h->stream));
        HIPCHK(h, hipEventSynchronize(ev[1]));
        HIPCHK(h, hipEventElapsedTime(&ms, ev[0], ev[1]));
        fprintf(stderr, "[apv norm2] n=%d count=%d method=%d: %.3f ms\n", n, count, method, ms);
    }
    HIPCHK(h, hipMemcpyAsync(h_out, dn, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

// gathers the leading `rank` columns of U [batch][n][n] into [batch][n][rank]
__global__ void __launch_bounds__(256) lead_cols_kernel(int n, int rank, const double* __restrict__ U, double* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)n * rank;
    if (idx >= per) return;
    const int z = blockIdx.y;
    const int i = (int)(idx / rank), j = (int)(idx % rank);
    out[z * per + idx] = U[(size_t)z * n * n + (size_t)i * n + j];
}

int apv_jdiag_leading(apv_handle* h, int32_t n, int32_t batch, int32_t rank, const double* h_A, const double* h_B, double* h_U,
                      double* h_lam, int32_t* h_info) {
    if (!h || !h_A || !h_B || !h_U || !h_lam) return fail(h, APV_ERR_ARG, "null host pointer");
    if (n < 1 || n > 4096 || batch < 0) return fail(h, APV_ERR_ARG, "apv_jdiag_leading: n must be in 1..4096");
    if (rank < 1 || rank > n) return fail(h, APV_ERR_ARG, "apv_jdiag_leading: rank must be in 1..n");
    if (batch == 0) return APV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t mat = (size_t)batch * n * n * sizeof(double);
    ApvOwned t;                                             // freed on every way out
    double *dA = nullptr, *dB = nullptr, *dU = nullptr, *dl = nullptr, *dn = nullptr, *dV = nullptr;
    HIPCHK(h, t.device(&dA, mat));
    HIPCHK(h, t.device(&dB, mat));
    HIPCHK(h, t.device(&dU, mat));
    HIPCHK(h, t.device(&dl, (size_t)batch * n * sizeof(double)));
    HIPCHK(h, t.device(&dV, (size_t)batch * n * rank * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(dA, h_A, mat, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dB, h_B, mat, hipMemcpyHostToDevice, h->stream));
    if (h->cfg.reg_mode == APV_REG_REL) {
        HIPCHK(h, t.device(&dn, (size_t)batch * sizeof(double)));
        for (int z0 = 0; z0 < batch; z0 += 4) {
            const double* mats[4];
            const int cnt = batch - z0 < 4 ? batch - z0 : 4;
            for (int q = 0; q < cnt; ++q) mats[q] = dB + (size_t)(z0 + q) * n * n;
            HIPCHK(h, apv_launch_norm2(n, cnt, mats, dn + z0, h->stream));
        }
    }
    std::vector<int32_t> st(batch, 0);
    h->gl_lead_rank = rank;
    int rc = apv_gevd_large(h, n, batch, dA, dB, h->cfg.reg_dark, dn, dU, dl, nullptr, 0.0, 0, nullptr, nullptr, st.data());
    const int lead_done = h->gl_lead_done;
    if (rc != APV_OK) return rc;
    const size_t per = (size_t)n * rank;
    hipLaunchKernelGGL(lead_cols_kernel, dim3((unsigned)((per + 255) / 256), batch), dim3(256), 0, h->stream, n, rank, dU, dV);
    HIPCHK(h, hipMemcpyAsync(h_U, dV, (size_t)batch * per * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    for (int z = 0; z < batch; ++z)
        HIPCHK(h, hipMemcpyAsync(h_lam + (size_t)z * rank, dl + (size_t)z * n, sizeof(double) * rank, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int z = 0; z < batch; ++z) {
        if (h_info) h_info[z] = lead_done ? 0 : 1;
        if (st[z] == 2) return fail(h, APV_ERR_NO_CONVERGE, "eigen-iteration did not converge");
    }
    return APV_OK;
}

// Evaluation: pressure at the microphones for given loudspeaker signals.  h_x [T][L], h_rir [P][L][M] (the
// (rir_len, L, M) layout of rirs.mat), h_out [T][M], all float64.      replaces predictPressure.m:1-17
int apv_predict_pressure(apv_handle* h, int32_t T, int32_t L, int32_t M, int32_t P, const double* h_x,
                         const double* h_rir, double* h_out) {
    if (!h || !h_x || !h_rir || !h_out) return fail(h, APV_ERR_ARG, "null argument");
    if (T < 0 || L < 1 || M < 1 || M > 256 || P < 1) return fail(h, APV_ERR_ARG, "predict_pressure: bad sizes (M <= 256)");
    if (T == 0) return APV_OK;
    HIPCHK(h, hipSetDevice(h->device));
    ApvOwned tmp;                                           // freed on every way out
    double *dx = nullptr, *dr = nullptr, *dout = nullptr;
    HIPCHK(h, tmp.device(&dx, sizeof(double) * (size_t)T * L));
    HIPCHK(h, tmp.device(&dr, sizeof(double) * (size_t)P * L * M));
    HIPCHK(h, tmp.device(&dout, sizeof(double) * (size_t)T * M));
    HIPCHK(h, hipMemcpyAsync(dx, h_x, sizeof(double) * (size_t)T * L, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dr, h_rir, sizeof(double) * (size_t)P * L * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, apv_launch_predict_pressure(T, L, M, P, dx, dr, dout, h->stream));
    HIPCHK(h, hipMemcpyAsync(h_out, dout, sizeof(double) * (size_t)T * M, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

// Static (signal-independent) VAST from the impulse responses alone.  h_gB [Nb][P][L], h_gD [Nd][P][L] (the
// (mics, rirLength, sources) layout of vast.m), h_w [J L].               replaces Matlab/ControlMethods/vast.m:46-91
int apv_vast_static(apv_handle* h, int32_t Nb, int32_t Nd, int32_t P, int32_t L, int32_t J, int32_t modeling_delay,
                    int32_t reference_index, int32_t V, double mu, const double* h_gB, const double* h_gD, double* h_w) {
    if (!h || !h_gB || !h_gD || !h_w) return fail(h, APV_ERR_ARG, "null argument");
    const int n = J * L;
    if (Nb < 1 || Nd < 1 || P < 1 || L < 1 || J < 1 || n > 4096 || V < 1 || V > n || modeling_delay < 0 || modeling_delay >= P ||
        reference_index < 0 || reference_index >= L || P <= J)
        return fail(h, APV_ERR_ARG, "vast_static: bad sizes (J L <= 4096, rir_len > J)");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    // vast.m drives the filters with a unit impulse for N = 1000 steps (vast.m:50-53): 999 of them are non-trivial
    const int ncols = 999, S = ncols + J;
    auto pack = [&](const double* g, int Nm, std::vector<double>& out) {          // [m*L + s][S], g'[u] = g[u-(J-1)]
        out.assign((size_t)Nm * L * S, 0.0);
        for (int m = 0; m < Nm; ++m)
            for (int sI = 0; sI < L; ++sI)
                for (int q = 0; q < P && q + J - 1 < S; ++q)
                    out[((size_t)m * L + sI) * S + q + J - 1] = g[((size_t)m * P + q) * L + sI];
    };
    std::vector<double> sb, sd, td((size_t)Nb * S, 0.0);
    pack(h_gB, Nb, sb);
    pack(h_gD, Nd, sd);
    for (int m = 0; m < Nb; ++m)                                                   // target: delayed reference RIR (vast.m:59)
        for (int q = modeling_delay; q < P && J + q < S; ++q)
            td[(size_t)m * S + J + q] = h_gB[((size_t)m * P + (q - modeling_delay)) * L + reference_index];
    ApvOwned tmp;                                           // freed on every way out
    double *dsb = nullptr, *dsd = nullptr, *dtd = nullptr, *dR = nullptr, *dr = nullptr, *dU = nullptr, *dl = nullptr, *dw = nullptr;
    HIPCHK(h, tmp.device(&dsb, sizeof(double) * sb.size()));
    HIPCHK(h, tmp.device(&dsd, sizeof(double) * sd.size()));
    HIPCHK(h, tmp.device(&dtd, sizeof(double) * td.size()));
    HIPCHK(h, tmp.device(&dR, sizeof(double) * 2 * (size_t)n * n));
    HIPCHK(h, tmp.device(&dr, sizeof(double) * n));
    HIPCHK(h, tmp.device(&dU, sizeof(double) * (size_t)n * n));
    HIPCHK(h, tmp.device(&dl, sizeof(double) * n));
    HIPCHK(h, tmp.device(&dw, sizeof(double) * (size_t)V * n));
    HIPCHK(h, hipMemcpyAsync(dsb, sb.data(), sizeof(double) * sb.size(), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(dsd, sd.data(), sizeof(double) * sd.size(), hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(dtd, td.data(), sizeof(double) * td.size(), hipMemcpyHostToDevice, st));
    {
        SyrkJobs jb{}, jd{};
        jb.stats[0] = dsb; jb.R[0] = dR;
        jd.stats[0] = dsd; jd.R[0] = dR + (size_t)n * n;
        HIPCHK(h, apv_launch_syrk_hankel(st, n, J, L, Nb, S, 0, 0, S - J, 1, jb));
        HIPCHK(h, apv_launch_syrk_hankel(st, n, J, L, Nd, S, 0, 0, S - J, 1, jd));
    }
    HIPCHK(h, apv_launch_xcorr_hankel(n, J, L, Nb, S, 0, 0, S - J, J, dsb, dtd, dr, st));
    // vast.m:71-73 normalises all three by numberOfMics (of the BRIGHT zone) * (rirLength - filterLength)
    const double f = 1.0 / ((double)Nb * (double)(P - J));
    const size_t nn = (size_t)n * n;
    HIPCHK(h, apv_launch_scale_f64(2 * nn, dR, f, st));
    HIPCHK(h, apv_launch_scale_f64((size_t)n, dr, f, st));
    int32_t status = 0;
    int rc = apv_gevd_large(h, n, 1, dR, dR + nn, 0.0, nullptr, dU, dl, dr, mu, V, nullptr, dw, &status);     // jdiag(RB, RD, 'vector', true): no loading
    if (rc == APV_OK) {
        (void)hipMemcpyAsync(h_w, dw + (size_t)(V - 1) * n, sizeof(double) * n, hipMemcpyDeviceToHost, st);
        (void)hipStreamSynchronize(st);
    }
    if (rc == APV_OK && status == 2)
        return fail(h, APV_ERR_NO_CONVERGE, "vast_static: eigen-iteration did not converge (Jacobi sweep cap reached); w was written");
    return rc;
}

// The Hankel statistics of the broadband stream and of the static solver on host buffers, either form on request
// (kernels_bb.hip: hankel_corr_kernel / syrk_hankel_kernel, xcorr_hankel_kernel); sizes checked as apv_bb_init checks them.
int apv_hankel_statistics(apv_handle* h, int32_t J, int32_t L, int32_t M, int32_t S, int32_t off, int32_t skip, int32_t ncols,
                          int32_t toff, int32_t njobs, const double* h_stats, const double* h_tstats, int32_t form,
                          double* h_R, double* h_r, int32_t* form_taken) {
    if (!h || !h_stats || !h_R) return fail(h, APV_ERR_ARG, "null argument");
    if (h_tstats && !h_r) return fail(h, APV_ERR_ARG, "apv_hankel_statistics: h_tstats without h_r");
    if (njobs < 1 || njobs > 4) return fail(h, APV_ERR_ARG, "apv_hankel_statistics: njobs must be in 1..4");
    if (form != APV_HANKEL_AUTO && form != APV_HANKEL_DISPLACEMENT && form != APV_HANKEL_DENSE)
        return fail(h, APV_ERR_ARG, "apv_hankel_statistics: unknown form");
    if (J < 1 || L < 1 || M < 1 || S < 1 || (long long)J * L > 4096)
        return fail(h, APV_ERR_ARG, "apv_hankel_statistics: bad sizes (1 <= J, J L <= 4096)");
    if (off < 0 || off >= S || (skip != 0 && skip != 1) || ncols < 1 || (long long)ncols + J - 1 + skip > S || toff < 0 ||
        (long long)toff + ncols > S)
        return fail(h, APV_ERR_ARG, "apv_hankel_statistics: off, skip, ncols or toff out of range for the ring length");
    const int n = J * L;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t per = (size_t)M * L * S, nn = (size_t)n * n;
    ApvOwned tmp;                                           // freed on every way out
    double *ds = nullptr, *dt = nullptr, *dR = nullptr, *dr = nullptr;
    HIPCHK(h, tmp.device(&ds, sizeof(double) * per * njobs));
    HIPCHK(h, tmp.device(&dR, sizeof(double) * nn * njobs));
    HIPCHK(h, hipMemcpyAsync(ds, h_stats, sizeof(double) * per * njobs, hipMemcpyHostToDevice, st));
    if (h_tstats) {
        HIPCHK(h, tmp.device(&dt, sizeof(double) * (size_t)M * S));
        HIPCHK(h, tmp.device(&dr, sizeof(double) * n));
        HIPCHK(h, hipMemcpyAsync(dt, h_tstats, sizeof(double) * (size_t)M * S, hipMemcpyHostToDevice, st));
    }
    SyrkJobs jobs{};
    for (int q = 0; q < njobs; ++q) {
        jobs.stats[q] = ds + q * per;
        jobs.R[q] = dR + q * nn;
    }
    int taken = 0;
    const hipError_t e = apv_launch_syrk_hankel(st, n, J, L, M, S, off, skip, ncols, njobs, jobs, form, &taken);
    if (e == hipErrorInvalidValue && form == APV_HANKEL_DISPLACEMENT && !taken)
        return fail(h, APV_ERR_ARG, "apv_hankel_statistics: the displacement form does not fit these sizes (2 J - 1 <= 1024, LDS <= 158 KiB)");
    HIPCHK(h, e);
    if (h_tstats) HIPCHK(h, apv_launch_xcorr_hankel(n, J, L, M, S, off, skip, ncols, toff, ds, dt, dr, st));
    HIPCHK(h, hipMemcpyAsync(h_R, dR, sizeof(double) * nn * njobs, hipMemcpyDeviceToHost, st));
    if (h_tstats) HIPCHK(h, hipMemcpyAsync(h_r, dr, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (form_taken) *form_taken = taken;
    return APV_OK;
}

int apv_stft_analysis_dev(apv_handle* h, int32_t n_ch, const float* d_x, void* d_spec) {
    if (!h || !d_x || !d_spec) return fail(h, APV_ERR_ARG, "null device pointer");
    if (h->cfg.block_size <= 0) return fail(h, APV_ERR_ARG, "handle was created without an STFT geometry");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    std::string why;
    hipError_t e = apv_launch_stft_analysis(h->cfg.block_size, n_ch, d_x, (float2*)d_spec, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_istft_ola_dev(apv_handle* h, int32_t n_ch, const void* d_spec, float* d_overlap, float* d_out) {
    if (!h || !d_spec || !d_overlap) return fail(h, APV_ERR_ARG, "null device pointer");
    if (h->cfg.block_size <= 0) return fail(h, APV_ERR_ARG, "handle was created without an STFT geometry");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    std::string why;
    hipError_t e = apv_launch_istft_ola(h->cfg.block_size, h->cfg.hop_size, n_ch, (const float2*)d_spec, d_overlap,
                                        d_out, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

// The transforms as the streams launch them (any precision, strides, zero padding, ring offset, channel sets, chunk form).  The
// kernels take their arguments on trust; what could make them read or write outside the caller's buffers is refused here.
namespace {
bool transform_refused(apv_handle* h, int32_t f64, std::string* msg) {    // the handle's block size has no plan in this precision
    if (h->cfg.block_size <= 0) *msg = "handle was created without an STFT geometry";
    else if (apv_stft_size_ok(h->cfg.block_size, msg) && f64 && h->cfg.block_size > 4096)
        *msg = "float64 transforms: block_size <= 4096 (double-precision FFT in LDS)";
    return !msg->empty();
}
int transform_done(apv_handle* h, hipError_t e, const std::string& why) {
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP, why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}
}  // namespace

int apv_analysis_dev(apv_handle* h, int32_t f64, int32_t n_ch, const void* d_x, int64_t x_stride, int32_t in_len,
                     int32_t ring_off, int32_t use_win, void* d_spec, int64_t stride_c, int64_t stride_k) {
    if (!h || !d_x || !d_spec) return fail(h, APV_ERR_ARG, "null device pointer");
    if (std::string msg; transform_refused(h, f64, &msg)) return fail(h, APV_ERR_ARG, msg);
    const int N = h->cfg.block_size;
    if (n_ch < 0) return fail(h, APV_ERR_ARG, "apv_analysis_dev: n_ch must not be negative");
    if (in_len < 0 || in_len > N) return fail(h, APV_ERR_ARG, "apv_analysis_dev: in_len must be in 0..block_size");
    if (x_stride < in_len) return fail(h, APV_ERR_ARG, "apv_analysis_dev: x_stride must be at least in_len");
    if (ring_off % N != 0 && (in_len != N || x_stride < N))
        return fail(h, APV_ERR_ARG, "apv_analysis_dev: a ring offset needs in_len == block_size and x_stride >= block_size");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    std::string why;
    return transform_done(h, apv_launch_analysis(f64 ? 1 : 0, N, n_ch, d_x, (long)x_stride, in_len, ring_off, use_win ? 1 : 0, d_spec,
                                                 (long)stride_c, (long)stride_k, h->stream, &why), why);
}

int apv_analysis_jobs_dev(apv_handle* h, int32_t f64, int32_t n_jobs, const void* const* d_x, const int32_t* n_ch,
                          void* const* d_spec, const int64_t* stride_c, const int64_t* stride_k, int32_t ring_off,
                          int32_t n_hops, int64_t x_stride, int64_t x_hop, const int64_t* spec_hop) {
    if (!h || !d_x || !n_ch || !d_spec || !stride_c || !stride_k) return fail(h, APV_ERR_ARG, "null argument");
    if (std::string msg; transform_refused(h, f64, &msg)) return fail(h, APV_ERR_ARG, msg);
    const int N = h->cfg.block_size;
    if (n_jobs < 1 || n_jobs > APV_STFT_MAX_JOBS) return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: n_jobs must be in 1..8");
    if (n_hops < 0 || n_hops > 65535) return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: n_hops must be in 0..65535");
    const void* x[APV_STFT_MAX_JOBS];
    void* spec[APV_STFT_MAX_JOBS];
    int nc[APV_STFT_MAX_JOBS];
    long sc[APV_STFT_MAX_JOBS], sk[APV_STFT_MAX_JOBS], sh[APV_STFT_MAX_JOBS];
    for (int j = 0; j < n_jobs; ++j) {
        if (n_ch[j] < 0) return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: n_ch must not be negative");
        if (n_ch[j] > 0 && (!d_x[j] || !d_spec[j])) return fail(h, APV_ERR_ARG, "null device pointer");
        if (stride_c[j] < 1 || stride_k[j] < 1) return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: strides must be at least 1");
        x[j] = d_x[j]; spec[j] = d_spec[j]; nc[j] = n_ch[j];
        sc[j] = (long)stride_c[j]; sk[j] = (long)stride_k[j]; sh[j] = spec_hop ? (long)spec_hop[j] : 0;
    }
    if (n_hops >= 1) {
        if (ring_off != 0) return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: the chunk form reads linear rows (ring_off must be 0)");
        if (x_hop < 0 || x_stride < N + (int64_t)(n_hops - 1) * x_hop)
            return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: x_stride must hold block_size + (n_hops - 1) x_hop samples");
        if (n_hops > 1 && !spec_hop) return fail(h, APV_ERR_ARG, "apv_analysis_jobs_dev: spec_hop is needed with more than one hop");
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    std::string why;
    const hipError_t e = n_hops >= 1 ? apv_launch_stft_analysis_chunk(f64 ? 1 : 0, N, n_jobs, x, nc, spec, sc, sk, (long)x_stride, (long)x_hop,
                                                                      sh, n_hops, h->stream, &why)
                                     : apv_launch_stft_analysis_jobs(f64 ? 1 : 0, N, n_jobs, x, nc, spec, sc, sk, ring_off, h->stream, &why);
    return transform_done(h, e, why);
}

int apv_synthesis_dev(apv_handle* h, int32_t f64, int32_t n_ch, const void* d_spec, int64_t stride_c, int64_t stride_k,
                      void* d_overlap, void* d_out, int32_t out_group, int64_t out_gstride) {
    if (!h || !d_spec || !d_overlap) return fail(h, APV_ERR_ARG, "null device pointer");
    if (std::string msg; transform_refused(h, f64, &msg)) return fail(h, APV_ERR_ARG, msg);
    const int N = h->cfg.block_size, H = h->cfg.hop_size;
    if (n_ch < 0) return fail(h, APV_ERR_ARG, "apv_synthesis_dev: n_ch must not be negative");
    if (out_group < 0) return fail(h, APV_ERR_ARG, "apv_synthesis_dev: out_group must not be negative");
    if (out_gstride != 0 && out_gstride < (int64_t)H * out_group)
        return fail(h, APV_ERR_ARG, "apv_synthesis_dev: out_gstride must be 0 or at least hop_size * out_group");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    std::string why;
    return transform_done(h, apv_launch_synthesis(f64 ? 1 : 0, N, H, n_ch, d_spec, (long)stride_c, (long)stride_k, d_overlap, d_out,
                                                  h->stream, &why, out_group, (long)out_gstride), why);
}

int apv_constrain_filters(apv_handle* h, void* d_w, int32_t n_bins, int32_t nV, int32_t L, int32_t N, int32_t J, void* d_taps) {
    if (!h || !d_w) return fail(h, APV_ERR_ARG, "null device pointer");
    if (N < 4 || (N & 1) || n_bins != N / 2 + 1) return fail(h, APV_ERR_ARG, "apv_constrain_filters: n_bins must be N / 2 + 1, N even");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    std::string why;
    void* w[1] = {d_w};
    void* taps[1] = {d_taps};
    hipError_t e = apv_launch_constrain_filters(h->cfg.out_c128, N, J, nV, L, 1, w, taps, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_limit_effort(apv_handle* h, int32_t c128, int32_t n_hops, int32_t K, int32_t nV, int32_t L, void* h_w, const double* h_limit,
                     double* h_effort, int32_t* h_rank, double* h_gain) {
    if (!h || !h_w || !h_limit) return fail(h, APV_ERR_ARG, "apv_limit_effort: null argument");
    if (n_hops < 1 || K < 1 || nV < 1 || L < 1) return fail(h, APV_ERR_ARG, "apv_limit_effort: n_hops, K, nV and L must be at least 1");
    for (int32_t k = 0; k < K; ++k)
        if (!(h_limit[k] > 0.0)) return fail(h, APV_ERR_ARG, "apv_limit_effort: a limit must be > 0 (+inf: no limit), not NaN");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    ApvOwned t;                                             // freed on every way out
    const size_t nb = (size_t)n_hops * K, wbytes = nb * nV * L * (c128 ? 16 : 8);
    char* dw = nullptr;
    double *dlim = nullptr, *deff = nullptr, *dgain = nullptr;
    int32_t* dsrc = nullptr;
    HIPCHK(h, t.device(&dw, wbytes));
    HIPCHK(h, t.device(&dlim, sizeof(double) * K));
    HIPCHK(h, t.device(&deff, sizeof(double) * nb * nV));
    HIPCHK(h, t.device(&dsrc, sizeof(int32_t) * nb));
    HIPCHK(h, t.device(&dgain, sizeof(double) * nb));
    HIPCHK(h, hipMemcpyAsync(dw, h_w, wbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dlim, h_limit, sizeof(double) * K, hipMemcpyHostToDevice, h->stream));
    EffortArgs a;
    a.w[0] = dw; a.limit[0] = dlim; a.effort[0] = deff; a.src[0] = dsrc; a.gain[0] = dgain;
    a.n_hops = n_hops;
    a.hop_w = (size_t)K * nV * L;
    a.emit_hop = EFFORT_EMIT_ALL;
    a.hop_bins = K;
    std::string why;
    hipError_t e = apv_launch_limit_effort(c128 != 0, K, nV, L, a, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    HIPCHK(h, hipMemcpyAsync(h_w, dw, wbytes, hipMemcpyDeviceToHost, h->stream));
    if (h_effort) HIPCHK(h, hipMemcpyAsync(h_effort, deff, sizeof(double) * nb * nV, hipMemcpyDeviceToHost, h->stream));
    if (h_rank) HIPCHK(h, hipMemcpyAsync(h_rank, dsrc, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, h->stream));
    if (h_gain) HIPCHK(h, hipMemcpyAsync(h_gain, dgain, sizeof(double) * nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return APV_OK;
}

int apv_validation_span(apv_handle* h, int32_t c128, int32_t K, int32_t nV, int32_t L, int32_t Mv, void* h_w, const void* h_G_bright,
                        const void* h_G_dark, const double* h_phi, double* h_bright, double* h_dark, int32_t* h_src, int32_t* h_rank,
                        int64_t* h_guard, float* h_ms) {
    if (!h || !h_w || !h_G_bright || !h_G_dark || !h_phi) return fail(h, APV_ERR_ARG, "apv_validation_span: null argument");
    if (K < 1 || nV < 1 || L < 1 || Mv < 1) return fail(h, APV_ERR_ARG, "apv_validation_span: K, nV, L and Mv must be at least 1");
    if (nV > APV_VALSPAN_MAX_SLOTS || L > APV_MAX_SRCS) return fail(h, APV_ERR_ARG, "apv_validation_span: nV and L are at most 128");
    for (int32_t k = 0; k < K; ++k)
        if (!(h_phi[k] >= 0.0) || !std::isfinite(h_phi[k]))
            return fail(h, APV_ERR_ARG, "apv_validation_span: a floor must be finite and >= 0 (0: no floor), not NaN");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    ApvOwned t;                                             // freed on every way out
    // every device buffer of the call lies between two guard bands of GUARD bytes of 0xA5; h_guard counts the guard bytes that
    // hold anything else after the launch
    constexpr size_t GUARD = 512;
    struct Band { unsigned char* base; size_t bytes; };
    std::vector<Band> bands;
    auto guarded = [&](auto** p, size_t bytes) -> hipError_t {
        unsigned char* base = nullptr;
        hipError_t e = t.device(&base, bytes + 2 * GUARD);
        if (e != hipSuccess) return e;
        e = hipMemsetAsync(base, 0xA5, bytes + 2 * GUARD, h->stream);
        *p = reinterpret_cast<std::remove_reference_t<decltype(*p)>>(base + GUARD);
        bands.push_back({base, bytes});
        return e;
    };
    const size_t nw = (size_t)K * nV * L, wbytes = nw * (c128 ? 16 : 8), gbytes = (size_t)K * Mv * L * 16, no = (size_t)K * nV;
    char *dw = nullptr, *dgb = nullptr, *dgd = nullptr;
    double *dphi = nullptr, *dbright = nullptr, *ddark = nullptr;
    int32_t* dsrc = nullptr;
    HIPCHK(h, guarded(&dw, wbytes));
    HIPCHK(h, guarded(&dgb, gbytes));
    HIPCHK(h, guarded(&dgd, gbytes));
    HIPCHK(h, guarded(&dphi, sizeof(double) * K));
    HIPCHK(h, guarded(&dbright, sizeof(double) * no));
    HIPCHK(h, guarded(&ddark, sizeof(double) * no));
    HIPCHK(h, guarded(&dsrc, sizeof(int32_t) * no));
    HIPCHK(h, hipMemcpyAsync(dw, h_w, wbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dgb, h_G_bright, gbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dgd, h_G_dark, gbytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dphi, h_phi, sizeof(double) * K, hipMemcpyHostToDevice, h->stream));
    ValSpanArgs a;
    a.w[0] = dw; a.g_bright[0] = dgb; a.g_dark[0] = dgd; a.phi[0] = dphi; a.bright[0] = dbright; a.dark[0] = ddark; a.src[0] = dsrc;
    std::string why;
    if (h_ms) HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    hipError_t e = apv_launch_validation_span(c128 != 0, K, nV, L, Mv, a, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    if (h_ms) HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    std::vector<int32_t> src(no);
    HIPCHK(h, hipMemcpyAsync(h_w, dw, wbytes, hipMemcpyDeviceToHost, h->stream));
    if (h_bright) HIPCHK(h, hipMemcpyAsync(h_bright, dbright, sizeof(double) * no, hipMemcpyDeviceToHost, h->stream));
    if (h_dark) HIPCHK(h, hipMemcpyAsync(h_dark, ddark, sizeof(double) * no, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(src.data(), dsrc, sizeof(int32_t) * no, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h_src) std::copy(src.begin(), src.end(), h_src);
    if (h_rank)
        for (int32_t k = 0; k < K; ++k) h_rank[k] = src[(size_t)k * nV + nV - 1] + 1;       // ranks 1 .. nV; 0: no source
    if (h_ms) HIPCHK(h, hipEventElapsedTime(h_ms, h->ev0, h->ev1));
    if (h_guard) {
        std::vector<unsigned char> g(2 * GUARD);
        int64_t bad = 0;
        for (const Band& b : bands) {
            HIPCHK(h, hipMemcpy(g.data(), b.base, GUARD, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemcpy(g.data() + GUARD, b.base + GUARD + b.bytes, GUARD, hipMemcpyDeviceToHost));
            for (unsigned char v : g) bad += v != 0xA5;
        }
        *h_guard = bad;
    }
    return APV_OK;
}

int apv_fir_synthesis(apv_handle* h, const void* d_x, const void* d_taps_prev, const void* d_taps_cur, int32_t nV, int32_t L,
                      int32_t J, int32_t H, void* d_out) {
    if (!h || !d_x || !d_taps_prev || !d_taps_cur || !d_out) return fail(h, APV_ERR_ARG, "null device pointer");
    if (J < 1 || H < 1 || nV < 1 || L < 1) return fail(h, APV_ERR_ARG, "apv_fir_synthesis: J, H, nV and L must be at least 1");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    const apv_config& c = h->cfg;
    const int x_f64 = c.frontend == 1 ? 0 : c.frontend == 2 ? 1 : c.compute_dtype == APV_F64;
    const size_t esz = x_f64 ? 8 : 4;
    FirSynthArgs a{};
    a.prev[0] = d_taps_prev; a.cur[0] = d_taps_cur; a.sig[0] = 0;
    a.xhist[0] = d_x; a.xhop[0] = static_cast<const char*>(d_x) + (size_t)(J - 1) * esz;
    a.nz = 1; a.nV = nV; a.L = L; a.J = J; a.H = H;
    a.n_tgt = 0;
    a.out = d_out; a.sn = L; a.sl = 1;
    std::string why;
    hipError_t e = apv_launch_fir_synthesis(c.out_c128, x_f64, a, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_eval_pressure(apv_handle* h, const void* d_y, const double* d_rv, int32_t G, int32_t L, int32_t Pv, int32_t H, int32_t Mv,
                      double* d_p) {
    if (!h || !d_y || !d_rv || !d_p) return fail(h, APV_ERR_ARG, "null device pointer");
    if (G < 1 || L < 1 || Pv < 1 || H < 1 || Mv < 1) return fail(h, APV_ERR_ARG, "apv_eval_pressure: G, L, Pv, H and Mv must be at least 1");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    const apv_config& c = h->cfg;
    const int x_f64 = c.frontend == 1 ? 0 : c.frontend == 2 ? 1 : c.compute_dtype == APV_F64;
    const size_t esz = x_f64 ? 8 : 4;
    EvalPressureArgs a{};
    a.hist = d_y; a.hop = static_cast<const char*>(d_y) + (size_t)(Pv - 1) * L * esz;
    a.hist_stride = a.hop_stride = ((size_t)Pv - 1 + H) * L;
    a.sn = L; a.sl = 1;
    a.rv[0] = d_rv; a.map = nullptr; a.p = d_p;
    a.n_sets = G; a.Pv = Pv; a.H = H; a.L = L; a.Mv = Mv;
    std::string why;
    hipError_t e = apv_launch_eval_pressure(x_f64, a, h->stream, &why);
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_eval_energies(apv_handle* h, const double* d_p, int32_t Z, int32_t E, int32_t H, int32_t Mv, int32_t n_hops, double* d_record,
                      double* d_totals) {
    if (!h || !d_p || !d_record || !d_totals) return fail(h, APV_ERR_ARG, "apv_eval_energies: null device pointer");
    std::string why;
    if (!apv_bbeval_sizes_ok(Z, E, H, Mv, n_hops, &why)) return fail(h, APV_ERR_ARG, why);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    BbEvalEnergyArgs a{};
    a.p = d_p; a.rec = d_record; a.slot0 = 0;
    a.Z = Z; a.E = E; a.H = H; a.Mv = Mv; a.n = n_hops;
    hipError_t e = apv_launch_bbeval_energies(a, h->stream, &why);
    if (e == hipSuccess) {
        BbEvalAdvanceArgs adv{};
        adv.rec = d_record; adv.totals = d_totals;
        adv.slot0 = 0; adv.Z = Z; adv.E = E; adv.H = H; adv.Mv = Mv; adv.n = n_hops; adv.Pv = 1; adv.L = 1; adv.n_hist = 0;
        e = apv_launch_bbeval_advance(adv, h->stream);
    }
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_eval_spectrum_step(apv_handle* h, const double* d_pressure, double* d_ring, int32_t ring_off, int32_t N, int32_t H, int32_t Z,
                           int32_t E, int32_t Mv, double* d_totals) {
    if (!h || !d_pressure || !d_ring || !d_totals) return fail(h, APV_ERR_ARG, "null device pointer");
    if (N < 1 || H < 1 || Z < 1 || E < 1 || Mv < 1) return fail(h, APV_ERR_ARG, "apv_eval_spectrum_step: N, H, Z, E and Mv must be at least 1");
    if ((N & 1) || N > 4096) return fail(h, APV_ERR_ARG, "apv_eval_spectrum_step: N must be even and at most 4096 (float64 transforms)");
    if (ring_off < 0 || ring_off >= N) return fail(h, APV_ERR_ARG, "apv_eval_spectrum_step: ring_off must be in 0..N - 1");
    std::string why;
    if (!apv_eval_spectra_size_ok(N, H, Z, E, Mv, &why)) return fail(h, APV_ERR_ARG, why);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    HIPCHK(h, apv_stft_prepare(N, 1));
    // the bin-major scratch of the transform is this call's own: a test entry, not a per-hop path
    ApvOwned t;
    void* spec = nullptr;
    HIPCHK(h, t.device(&spec, sizeof(double) * 2 * ((size_t)N / 2 + 1) * Z * (2 * (size_t)E + 1) * Mv));
    EvalSpectraArgs a{};
    a.p = d_pressure; a.ring = d_ring; a.spec = spec; a.totals = d_totals;
    a.ring_off = ring_off; a.N = N; a.H = H; a.Z = Z; a.E = E; a.Mv = Mv;
    hipError_t e = apv_launch_eval_spectra(a, h->stream, &why);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_eval_spectra_hops(apv_handle* h, const double* d_pressure, double* d_tail, int32_t N, int32_t H, int32_t Z, int32_t E, int32_t Mv,
                          int32_t n_hops, int32_t hops_per_launch, double* d_totals) {
    if (!h || !d_pressure || !d_totals) return fail(h, APV_ERR_ARG, "apv_eval_spectra_hops: null device pointer");
    if (N < 1 || H < 1 || Z < 1 || E < 1 || Mv < 1 || n_hops < 1)
        return fail(h, APV_ERR_ARG, "apv_eval_spectra_hops: N, H, Z, E, Mv and n_hops must be at least 1");
    if ((N & 1) || N > 4096) return fail(h, APV_ERR_ARG, "apv_eval_spectra_hops: N must be even and at most 4096 (float64 transforms)");
    if (hops_per_launch < 0) return fail(h, APV_ERR_ARG, "apv_eval_spectra_hops: hops_per_launch must not be negative");
    if ((long long)n_hops * H > 0x7fffffffll) return fail(h, APV_ERR_ARG, "apv_eval_spectra_hops: n_hops x H must stay below 2^31");
    std::string why;
    if (!apv_bbspec_size_ok(N, H, Z, E, Mv, &why)) return fail(h, APV_ERR_ARG, why);
    if (H < N && !d_tail) return fail(h, APV_ERR_ARG, "apv_eval_spectra_hops: null tail with H < N");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    HIPCHK(h, apv_stft_prepare(N, 1));
    // lines and the transforms' scratch are this call's own: a test entry, not a per-hop path
    const int fit = apv_bbspec_hops_fit(N, Z, E, Mv), tail = N - H;
    const int c = std::min<int>(n_hops, hops_per_launch > 0 ? std::min<int>(hops_per_launch, fit) : fit);
    const size_t ch = (size_t)Z * (2 * (size_t)E + 1) * Mv, row = (size_t)tail + (size_t)c * H;
    ApvOwned t;
    BbSpecArgs a{};
    for (int b = 0; b < 2; ++b) HIPCHK(h, t.device(&a.line[b], sizeof(double) * ch * row));
    HIPCHK(h, t.device(&a.spec, sizeof(double) * 2 * (size_t)c * ((size_t)N / 2 + 1) * ch));
    // the tail alone is the line in front of the first hop
    if (tail > 0) HIPCHK(h, hipMemcpyAsync(a.line[0], d_tail, sizeof(double) * ch * tail, hipMemcpyDeviceToDevice, h->stream));
    a.p = d_pressure; a.p_set = (size_t)n_hops * H * Mv; a.cur = 0; a.len = tail; a.totals = d_totals;
    a.N = N; a.H = H; a.Z = Z; a.E = E; a.Mv = Mv; a.n = n_hops; a.per_launch = c;
    hipError_t e = apv_launch_bbspec_hops(&a, h->stream, &why);
    if (e == hipSuccess && tail > 0)
        e = hipMemcpy2DAsync(d_tail, sizeof(double) * tail, a.line[a.cur] + (a.len - tail), sizeof(double) * (size_t)a.len,
                             sizeof(double) * tail, ch, hipMemcpyDeviceToDevice, h->stream);
    const hipError_t es = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_eval_detect_step(apv_handle* h, const void* d_spec, int32_t N, int32_t Z, int32_t E, int32_t Mv, int32_t n_channels,
                         const double* h_G2, double Cs, double Ca, double Leff, double* d_hop, double* d_totals) {
    if (!h || !d_spec || !h_G2 || !d_hop || !d_totals) return fail(h, APV_ERR_ARG, "null pointer");
    if (N < 1 || Z < 1 || E < 1 || Mv < 1 || n_channels < 1)
        return fail(h, APV_ERR_ARG, "apv_eval_detect_step: N, Z, E, Mv and n_channels must be at least 1");
    if (N & 1) return fail(h, APV_ERR_ARG, "apv_eval_detect_step: N must be even");
    if (!std::isfinite(Cs) || !std::isfinite(Ca) || !std::isfinite(Leff) || !(Ca > 0.0))
        return fail(h, APV_ERR_ARG, "apv_eval_detect_step: Cs, Ca and Leff must be finite, Ca positive");
    std::string why;
    if (!apv_eval_detect_size_ok(N, Z, E, Mv, n_channels, &why)) return fail(h, APV_ERR_ARG, why);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    // the table, the curves and the partial sums are this call's own: a test entry, not a per-hop path
    const int K = N / 2 + 1, chunks = apv_eval_detect_chunks(N, Z, E, Mv);
    std::vector<double> gt((size_t)n_channels * K);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < n_channels; ++i) gt[(size_t)i * K + k] = h_G2[(size_t)k * n_channels + i];
    ApvOwned t;
    double *G2T = nullptr, *quiet = nullptr, *curves = nullptr, *part = nullptr;
    HIPCHK(h, t.device(&G2T, sizeof(double) * gt.size()));
    HIPCHK(h, t.device(&quiet, sizeof(double) * K));
    HIPCHK(h, t.device(&curves, sizeof(double) * (size_t)K * Z * Mv));
    HIPCHK(h, t.device(&part, sizeof(double) * (size_t)chunks * Z * 2 * E * Mv));
    HIPCHK(h, hipMemcpyAsync(G2T, gt.data(), sizeof(double) * gt.size(), hipMemcpyHostToDevice, h->stream));
    hipError_t e = apv_launch_eval_detect_quiet(N, n_channels, G2T, Cs, Ca, Leff, quiet, h->stream);
    if (e == hipSuccess) {
        EvalDetectArgs a{};
        a.spec = d_spec; a.G2T = G2T; a.quiet = quiet; a.curves = curves; a.part = part;
        a.hop = d_hop; a.ctl = nullptr; a.totals = d_totals;
        a.N = N; a.Z = Z; a.E = E; a.Mv = Mv; a.C = n_channels;
        a.Cs = Cs; a.Ca = Ca; a.Leff = Leff;
        e = apv_launch_eval_detect(a, h->stream, &why);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);  // gt and the scratch go out of scope
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_eval_detect_hops(apv_handle* h, const void* d_spec, int32_t n_hops, int32_t hops_per_launch, int32_t N, int32_t Z, int32_t E,
                         int32_t Mv, int32_t n_channels, const double* h_G2, double Cs, double Ca, double Leff, double* d_hops,
                         double* d_totals) {
    if (!h || !d_spec || !h_G2 || !d_hops || !d_totals) return fail(h, APV_ERR_ARG, "null pointer");
    if (N < 1 || Z < 1 || E < 1 || Mv < 1 || n_channels < 1 || n_hops < 1 || hops_per_launch < 1)
        return fail(h, APV_ERR_ARG, "apv_eval_detect_hops: N, Z, E, Mv, n_channels, n_hops and hops_per_launch must be at least 1");
    if (N & 1) return fail(h, APV_ERR_ARG, "apv_eval_detect_hops: N must be even");
    if (!std::isfinite(Cs) || !std::isfinite(Ca) || !std::isfinite(Leff) || !(Ca > 0.0))
        return fail(h, APV_ERR_ARG, "apv_eval_detect_hops: Cs, Ca and Leff must be finite, Ca positive");
    std::string why;
    if (!apv_eval_detect_size_ok(N, Z, E, Mv, n_channels, &why)) return fail(h, APV_ERR_ARG, why);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_join(h, true)) return rc;
    // the table, the curves and the partial sums are this call's own: a test entry, not a per-hop path
    const int K = N / 2 + 1, chunks = apv_eval_detect_chunks(N, Z, E, Mv), c = std::min<int>(std::min<int>(n_hops, hops_per_launch), 65535);
    std::vector<double> gt((size_t)n_channels * K);
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < n_channels; ++i) gt[(size_t)i * K + k] = h_G2[(size_t)k * n_channels + i];
    ApvOwned t;
    double *G2T = nullptr, *quiet = nullptr, *curves = nullptr, *part = nullptr;
    HIPCHK(h, t.device(&G2T, sizeof(double) * gt.size()));
    HIPCHK(h, t.device(&quiet, sizeof(double) * K));
    HIPCHK(h, t.device(&curves, sizeof(double) * (size_t)c * K * Z * Mv));
    HIPCHK(h, t.device(&part, sizeof(double) * (size_t)c * chunks * Z * 2 * E * Mv));
    HIPCHK(h, hipMemcpyAsync(G2T, gt.data(), sizeof(double) * gt.size(), hipMemcpyHostToDevice, h->stream));
    hipError_t e = apv_launch_eval_detect_quiet(N, n_channels, G2T, Cs, Ca, Leff, quiet, h->stream);
    if (e == hipSuccess) {
        BbSpecDetectArgs d{};
        d.G2T = G2T; d.quiet = quiet; d.curves = curves; d.part = part; d.rec = d_hops; d.totals = d_totals;
        d.slot0 = 0; d.C = n_channels; d.Cs = Cs; d.Ca = Ca; d.Leff = Leff;
        e = apv_launch_bbspec_detect_hops(d, d_spec, n_hops, c, N, Z, E, Mv, h->stream, &why);
    }
    const hipError_t es = hipStreamSynchronize(h->stream);  // gt and the scratch go out of scope
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(h, e == hipErrorInvalidValue ? APV_ERR_ARG : APV_ERR_HIP,
                                     why.empty() ? hipGetErrorString(e) : why);
    return APV_OK;
}

int apv_comm_unique_id(char id_out[128]) {
    if (!id_out) return APV_ERR_ARG;
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    if (ncclGetUniqueId(&id) != ncclSuccess) return APV_ERR_RCCL;
    std::memcpy(id_out, &id, 128);
    return APV_OK;
}

int apv_comm_init(apv_handle* h, const char id[128], int32_t rank, int32_t world) {
    if (!h || !id || world < 1 || rank < 0 || rank >= world) return fail(h, APV_ERR_ARG, "bad communicator arguments");
    HIPCHK(h, hipSetDevice(h->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, 128);
    ncclComm_t comm;
    ncclResult_t r = ncclCommInitRank(&comm, world, uid, rank);
    if (r != ncclSuccess) return fail(h, APV_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    // the communicator must be the one that was asked for: a rank that joined another job's id, or a world of another size,
    // would gather somebody else's shards without any call failing
    int count = -1, urank = -1;
    if (ncclCommCount(comm, &count) != ncclSuccess || ncclCommUserRank(comm, &urank) != ncclSuccess || count != world || urank != rank) {
        (void)ncclCommDestroy(comm);
        return fail(h, APV_ERR_RCCL, "communicator reports " + std::to_string(count) + " ranks / rank " + std::to_string(urank) +
                                         ", expected " + std::to_string(world) + " / " + std::to_string(rank));
    }
    h->comm = comm;
    h->comm_rank = rank;
    h->comm_world = world;
    if (!h->comm_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_ready, hipEventDisableTiming));
        for (auto& g : h->gather_done) HIPCHK(h, hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
        HIPCHK(h, hipEventCreate(&h->ev_ag0));
        HIPCHK(h, hipEventCreate(&h->ev_ag1));
        HIPCHK(h, hipMalloc((void**)&h->d_bar, sizeof(int32_t)));
        HIPCHK(h, hipMemset(h->d_bar, 0, sizeof(int32_t)));
    }
    return APV_OK;
}

int apv_allgather_filters_dev(apv_handle* h, const void* d_w_shard, void* d_w_all) {
    if (!h || !d_w_shard || !d_w_all) return fail(h, APV_ERR_ARG, "null device pointer");
    if (!h->comm) return fail(h, APV_ERR_RCCL, "communicator not initialised (apv_comm_init)");
    const apv_config& c = h->cfg;
    const size_t bytes = (size_t)c.n_bins * c.n_ranks * c.n_srcs * wsize(h);
    HIPCHK(h, hipSetDevice(h->device));
    // the gather starts once the kernels already queued on the compute stream have written the shard, and runs
    // on its own stream: the next block's update (into another shard buffer) overlaps it
    if (lanes_on(h)) {
        // the shard was written on a lane: the gather waits for the latest launch of BOTH lanes (whichever wrote it, now or
        // earlier; the other one's finished a step ago in the usual order of calls) -- on its own stream, so that no stream a
        // later launch could queue up behind carries the wait -- and for the control stream as below
        for (auto& ln : h->lane)
            if (ln.used) HIPCHK(h, hipStreamWaitEvent(h->comm_stream, ln.ev, 0));
    }
    HIPCHK(h, hipEventRecord(h->ev_ready, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_ready, 0));
    HIPCHK(h, hipEventRecord(h->ev_ag0, h->comm_stream));
    ncclResult_t r = ncclAllGather(d_w_shard, d_w_all, bytes, ncclChar, (ncclComm_t)h->comm, h->comm_stream);
    if (r != ncclSuccess) return fail(h, APV_ERR_RCCL, std::string("ncclAllGather: ") + ncclGetErrorString(r));
    HIPCHK(h, hipEventRecord(h->ev_ag1, h->comm_stream));
    h->ag_bytes = bytes;
    // remember "this shard buffer is being read until <event>": the slot already tracking this buffer, else a free one,
    // else the oldest -- whose gather the compute stream then waits for here, so no later update can overtake it
    int slot = -1;
    for (int i = 0; i < 4 && slot < 0; ++i)
        if (h->gather_done[i].ptr == d_w_shard) slot = i;
    for (int i = 0; i < 4 && slot < 0; ++i)
        if (h->gather_done[i].ptr == nullptr) slot = i;
    if (slot < 0) {
        slot = h->gather_next;
        h->gather_next = (h->gather_next + 1) & 3;
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->gather_done[slot].ev, 0));
        if (lanes_on(h))
            for (auto& ln : h->lane) HIPCHK(h, hipStreamWaitEvent(ln.s, h->gather_done[slot].ev, 0));
    }
    h->gather_done[slot].ptr = d_w_shard;
    HIPCHK(h, hipEventRecord(h->gather_done[slot].ev, h->comm_stream));
    return APV_OK;
}

int apv_host_alloc(void** p, size_t bytes) {
    if (!p) return APV_ERR_ARG;
    *p = nullptr;
    if (hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return APV_ERR_HIP;
    }
    apv_host_blocks_note(*p, bytes ? bytes : 1, true);
    return APV_OK;
}

int apv_host_free(void* p) {
    if (!p) return APV_OK;
    apv_host_blocks_note(p, 0, false);
    return hipHostFree(p) == hipSuccess ? APV_OK : APV_ERR_HIP;
}

int apv_comm_count(apv_handle* h, int32_t* n_ranks, int32_t* user_rank) {
    if (!h || !n_ranks) return fail(h, APV_ERR_ARG, "null argument");
    if (!h->comm) return fail(h, APV_ERR_RCCL, "communicator not initialised (apv_comm_init)");
    int count = 0, urank = 0;
    ncclResult_t r = ncclCommCount((ncclComm_t)h->comm, &count);
    if (r == ncclSuccess) r = ncclCommUserRank((ncclComm_t)h->comm, &urank);
    if (r != ncclSuccess) return fail(h, APV_ERR_RCCL, std::string("ncclCommCount: ") + ncclGetErrorString(r));
    *n_ranks = count;
    if (user_rank) *user_rank = urank;
    return APV_OK;
}

int apv_comm_last_gather(apv_handle* h, float* elapsed_ms, size_t* bytes_per_rank) {
    if (!h || !elapsed_ms) return fail(h, APV_ERR_ARG, "null argument");
    if (!h->comm || h->ag_bytes == 0) return fail(h, APV_ERR_RCCL, "no all-gather has run on this handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipEventSynchronize(h->ev_ag1));
    HIPCHK(h, hipEventElapsedTime(elapsed_ms, h->ev_ag0, h->ev_ag1));
    if (bytes_per_rank) *bytes_per_rank = h->ag_bytes;
    return APV_OK;
}

int apv_comm_barrier(apv_handle* h) {
    if (!h) return APV_ERR_ARG;
    if (!h->comm) return fail(h, APV_ERR_RCCL, "communicator not initialised (apv_comm_init)");
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = lanes_sync(h)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ncclResult_t r = ncclAllReduce(h->d_bar, h->d_bar, 1, ncclInt32, ncclSum, (ncclComm_t)h->comm, h->comm_stream);
    if (r != ncclSuccess) return fail(h, APV_ERR_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    HIPCHK(h, hipStreamSynchronize(h->comm_stream));
    return APV_OK;
}

int apv_debug_set_stamps(apv_handle* h, void* d_stamps) {
    if (!h) return APV_ERR_ARG;
    h->d_stamps = static_cast<unsigned long long*>(d_stamps);
    return APV_OK;
}

int apv_debug_live_resources(int32_t counts[4]) {
    if (!counts) return APV_ERR_ARG;
    for (int i = 0; i < 4; ++i) counts[i] = ApvOwned::live[i].load();
    return APV_OK;
}

int apv_device_sync(apv_handle* h) {
    if (!h) return APV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceSynchronize());
    return APV_OK;
}

int apv_device_info(apv_handle* h, char name_out[128], int32_t* n_cus, int32_t* clock_mhz) {
    if (!h || !name_out) return APV_ERR_ARG;
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, h->device));
    std::snprintf(name_out, 128, "%s (%s)", prop.name, prop.gcnArchName);
    if (n_cus) *n_cus = prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = prop.clockRate / 1000;
    return APV_OK;
}

}  // extern "C"
