// Owner of GPU resources: device buffers, page-locked host memory, events and streams are registered where they are made and
// freed together.  A stream state holds one for everything it keeps (apv_stream, apv_bb); a call holds a local one for its scratch,
// which then goes on every way out.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cassert>
#include <vector>

class ApvOwned {
public:
    ApvOwned() = default;
    ApvOwned(const ApvOwned&) = delete;
    ApvOwned& operator=(const ApvOwned&) = delete;
    ~ApvOwned() { clear(); }

    // what all owners of the process hold now: device buffers, pinned blocks, events, streams (apv_debug_live_resources)
    static inline std::atomic<int> live[4];

    template <typename T>
    hipError_t device(T** p, size_t bytes) { return keep(dev_, 0, p, hipMalloc((void**)p, bytes)); }
    // `count` elements (at least one) of `esz` bytes, zero-filled on `st`
    template <typename T>
    hipError_t zeroed(T** p, size_t count, size_t esz, hipStream_t st) {
        const size_t bytes = esz * (count ? count : 1);
        const hipError_t e = device(p, bytes);
        return e != hipSuccess ? e : hipMemsetAsync(*p, 0, bytes, st);
    }
    template <typename T>
    hipError_t pinned(T** p, size_t bytes) { return keep(pin_, 1, p, hipHostMalloc((void**)p, bytes, hipHostMallocDefault)); }
    hipError_t event(hipEvent_t* e, unsigned flags) { return keep(ev_, 2, e, hipEventCreateWithFlags(e, flags)); }
    hipError_t stream(hipStream_t* s, unsigned flags) { return keep(str_, 3, s, hipStreamCreateWithFlags(s, flags)); }
    hipError_t stream(hipStream_t* s, unsigned flags, int priority) {
        return keep(str_, 3, s, hipStreamCreateWithPriority(s, flags, priority));
    }

    // frees one registered buffer (device or pinned) ahead of the rest, where a call replaces it, and nulls the caller's pointer.
    // p is null or this owner's: a buffer made elsewhere would be lost here without a trace
    template <typename T>
    void release(T*& p) {
        auto it = std::find(dev_.begin(), dev_.end(), (void*)p);
        if (it != dev_.end()) {
            (void)hipFree(p);
            dev_.erase(it);
            --live[0];
        } else if ((it = std::find(pin_.begin(), pin_.end(), (void*)p)) != pin_.end()) {
            (void)hipHostFree(p);
            pin_.erase(it);
            --live[1];
        } else {
            assert(!p);
            return;
        }
        p = nullptr;
    }

    // device buffers first (hipFree waits for the device), then pinned memory, events, and the streams last
    void clear() {
        for (void* b : dev_) (void)hipFree(b);
        for (void* b : pin_) (void)hipHostFree(b);
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
        for (hipStream_t s : str_) (void)hipStreamDestroy(s);
        live[0] -= (int)dev_.size(); live[1] -= (int)pin_.size(); live[2] -= (int)ev_.size(); live[3] -= (int)str_.size();
        dev_.clear(); pin_.clear(); ev_.clear(); str_.clear();
    }

private:
    template <typename V, typename T>
    hipError_t keep(V& list, int kind, T* p, hipError_t e) {
        if (e != hipSuccess) {
            *p = nullptr;
            return e;
        }
        list.push_back(*p);
        ++live[kind];
        return hipSuccess;
    }
    std::vector<void*> dev_, pin_;
    std::vector<hipEvent_t> ev_;
    std::vector<hipStream_t> str_;
};
