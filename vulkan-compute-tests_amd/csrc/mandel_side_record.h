// Per-context records of the Mandelbrot features (the bound orbit, the equalised colouring's tables, the adaptive list).  Kept beside
// mc_context rather than in it so that mc_internal.h, which the path tracer's build id covers, stays as it is.
#pragma once
#include <mutex>
#include <unordered_map>

struct mc_context;

namespace mc {

// One map for every context (a context itself is used by one thread at a time): every access locks it.  A record's node stays put while
// other contexts add theirs; only its own context's thread erases it.
template <class Record>
class SideRecords {
public:
    Record* get(const mc_context* ctx) {   // the context's record, created on first use
        std::lock_guard<std::mutex> lock(mutex_);
        return &map_[ctx];
    }
    Record* find(const mc_context* ctx) {   // or nullptr
        std::lock_guard<std::mutex> lock(mutex_);
        auto it = map_.find(ctx);
        return it == map_.end() ? nullptr : &it->second;
    }
    template <class Release>
    void erase(const mc_context* ctx, Release release) {   // release(record) frees its device buffers first
        std::lock_guard<std::mutex> lock(mutex_);
        auto it = map_.find(ctx);
        if (it == map_.end()) return;
        release(it->second);
        map_.erase(it);
    }

private:
    std::mutex mutex_;
    std::unordered_map<const mc_context*, Record> map_;
};

}  // namespace mc
