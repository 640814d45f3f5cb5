// The pipeline's ordered placement (Landing, finito_amd/csrc/fin_host.h) under ThreadSanitizer, as a stand-alone program: no Python, no device, no HIP -- that
// header is all it takes.  From the repository root:
//   g++ -O1 -g -fsanitize=thread -std=c++17 -pthread -o /tmp/tsan_landing tools/tsan_landing.cpp
//   /tmp/tsan_landing
// (without the thread sanitizer's runtime: -fsanitize=address,undefined instead.)
// Eight threads take 64 sub-batches from a shared counter, as the pipeline's workers do, but dawdle by different amounts so that they place them in no particular
// order; every place() must return the sum of all earlier lengths, and total() their sum.  Then the same with one thread that gives up at its third sub-batch:
// every other thread must return from every place() it makes.  It prints "ok" and exits 0 when all of that held and the sanitizer reported nothing.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <thread>

#include "../finito_amd/csrc/fin_host.h"

static const size_t N_SUB = 64;
static const int N_THREADS = 8;
static uint64_t len_of(size_t i) { return (i * 2654435761u) % 1000 + (i % 7 == 0 ? 0 : 1); }   // (some sub-batches are empty)

// the run; `quitter` (-1: none) gives up when it has taken three sub-batches.  Returns the number of wrong offsets
static int run(int round, int quitter, uint64_t* total) {
    Landing land;
    land.reset(N_SUB);
    std::atomic<size_t> next{0};
    std::atomic<int> wrong{0};
    std::atomic<bool> failed{false};
    std::vector<std::thread> th;
    for (int t = 0; t < N_THREADS; t++)
        th.emplace_back([&, t] {
            int taken = 0;
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= N_SUB || failed.load()) break;
                if (t == quitter && ++taken == 3) { failed.store(true); land.give_up(); break; }
                std::this_thread::sleep_for(std::chrono::microseconds(((i * 7 + (size_t)t * 13 + (size_t)round * 5) % 11) * 50));   // later sub-batches often come first
                const uint64_t at = land.place(i, len_of(i));
                uint64_t want = 0;
                for (size_t j = 0; j < i; j++) want += len_of(j);
                if (quitter < 0 && at != want) wrong++;
            }
        });
    for (auto& x : th) x.join();   // (with a quitter: that every thread comes back is the check)
    *total = land.total();
    return wrong.load();
}

int main() {
    uint64_t sum = 0;
    for (size_t i = 0; i < N_SUB; i++) sum += len_of(i);
    for (int round = 0; round < 20; round++) {
        uint64_t total = 0;
        const int wrong = run(round, -1, &total);
        if (wrong || total != sum) { fprintf(stderr, "failed: round %d, %d wrong offsets, total %llu of %llu\n", round, wrong, (unsigned long long)total, (unsigned long long)sum); return 1; }
    }
    for (int quitter = 0; quitter < N_THREADS; quitter++) {
        uint64_t total = 0;
        (void)run(quitter, quitter, &total);
        if (total > sum) { fprintf(stderr, "failed: quitter %d, total %llu above %llu\n", quitter, (unsigned long long)total, (unsigned long long)sum); return 1; }
    }
    printf("ok\n");
    return 0;
}
