// work_pool_driver.cpp — stress of the host worker pool (biodemux.jl_amd/csrc/bdx_pool.h): many short back-to-back
// parallel_for sections of differing n (2..16, so the pool and the caller are at most 16 threads); every index of every
// section must run exactly once, and no index >= n may be called.  A watchdog ends the run when the section counter stops
// moving.  usage: work_pool_driver SECTIONS SECONDS  (ends at whichever limit comes first)
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "bdx_pool.h"

int main(int argc, char **argv) {
    const long sections = argc > 1 ? atol(argv[1]) : 1000000;
    const double seconds = argc > 2 ? atof(argv[2]) : 20.0;
    using clock = std::chrono::steady_clock;
    std::atomic<long> done{0};
    std::thread([&done]() {
        long last = -1;
        clock::time_point since = clock::now();
        for (;;) {
            std::this_thread::sleep_for(std::chrono::milliseconds(100));
            const long s = done.load();
            if (s != last) {
                last = s;
                since = clock::now();
            } else if (clock::now() - since > std::chrono::seconds(5)) {
                fprintf(stderr, "stall at section %ld\n", s);
                fflush(stderr);
                _exit(3);
            }
        }
    }).detach();
    std::atomic<int> hits[16];
    std::atomic<int> beyond{0};
    const clock::time_point t0 = clock::now();
    uint32_t rng = 12345;
    for (long s = 0; s < sections; ++s) {
        rng = rng * 1664525u + 1013904223u;
        const int n = 2 + (int)((rng >> 16) % 15);
        for (std::atomic<int> &h : hits) h.store(0);
        parallel_for(n, [&](const int i) {
            if (i < 0 || i >= n)
                beyond.fetch_add(1);
            else
                hits[i].fetch_add(1);
        });
        for (int i = 0; i < n; ++i)
            if (hits[i].load() != 1) {
                fprintf(stderr, "section %ld (n = %d): index %d ran %d times\n", s, n, i, hits[i].load());
                return 1;
            }
        if (beyond.load()) {
            fprintf(stderr, "section %ld (n = %d): %d calls with an index beyond n\n", s, n, beyond.load());
            return 2;
        }
        done.store(s + 1);
        if (std::chrono::duration<double>(clock::now() - t0).count() > seconds) break;
    }
    printf("work pool ok: %ld sections\n", done.load());
    return 0;
}
