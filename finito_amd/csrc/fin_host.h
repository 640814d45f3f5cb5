// fin_host.h -- host helpers shared by fin_capi.cpp and the host twins of fin_records_host.cpp.  Plain C++: no HIP header
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <condition_variable>
#include <mutex>
#include <vector>

// the first unitig of a colour matrix bits[n_unitigs][W] with a bit at or above n_colors set, or n_unitigs
static inline uint64_t colors_first_stray(const uint64_t* bits, uint64_t n_unitigs, uint32_t n_colors, uint32_t W) {
    if ((n_colors & 63u) == 0u) return n_unitigs;   // (the last word is all colours)
    const uint64_t stray = ~0ull << (n_colors & 63u);
    for (uint64_t u = 0; u < n_unitigs; u++) if (bits[u * W + (W - 1)] & stray) return u;
    return n_unitigs;
}

// Ordered placement: sub-batches of a read set finish in any order on several host threads, and what each made (text, pairs, segments) lands in ONE caller
// buffer behind what all earlier sub-batches made.  A sub-batch publishes its length and learns its place once every earlier length is known
struct Landing {
    void reset(size_t n_sub_batches) { len.assign(n_sub_batches, 0); known.assign(n_sub_batches, 0); }
    // publishes sub-batch i's length L and returns the sum of all earlier lengths once they are known (after give_up at once: the sum is then of no use, the
    // search has failed and the caller is about to learn it)
    uint64_t place(size_t i, uint64_t L) {
        std::unique_lock<std::mutex> g(mu);
        len[i] = L; known[i] = 1;
        cv.notify_all();
        cv.wait(g, [&] { for (size_t j = 0; j < i; j++) if (!known[j]) return false; return true; });
        uint64_t at = 0;
        for (size_t j = 0; j < i; j++) at += len[j];
        return at;
    }
    // a worker that fails will place none of its sub-batches: nobody may wait for them
    void give_up() {
        { std::lock_guard<std::mutex> g(mu); known.assign(known.size(), 1); }
        cv.notify_all();
    }
    uint64_t total() {
        std::lock_guard<std::mutex> g(mu);
        uint64_t t = 0;
        for (uint64_t l : len) t += l;
        return t;
    }
private:
    std::vector<uint64_t> len; std::vector<char> known;
    std::mutex mu; std::condition_variable cv;
};
