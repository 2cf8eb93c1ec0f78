// bdx_pool.h — the host side's one worker pool (plain C++17, no HIP: bdx_io.cpp and the HIP library both use it).
// The parallel sections of the native FASTQ reader / writer (line index, packer, sizes, gather, files) and of the host
// entry point (offset scan, window gather, result copies) run on a pool that belongs to the CALLING thread (the pipeline's
// reader and writer threads each keep their own for the whole run) instead of starting and joining a set of std::threads
// per section: a 10 M-read run has ~140 sections per stage, i.e. ~2 200 thread starts at a few tens of microseconds each
// on the coordinating thread.  Tasks are claimed with an atomic counter; the caller works too.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

class WorkPool {
  public:
    ~WorkPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_start_.notify_all();
        for (auto &t : th_) t.join();
    }
    // runs f(0) .. f(n - 1), each exactly once, and returns when all have returned
    template <class F>
    void run(int n, F &&f) {
        if (n <= 1) {
            if (n == 1) f(0);
            return;
        }
        try {
            while ((int)th_.size() < n - 1) th_.emplace_back([this]() { worker(); });
        } catch (...) {  // (no more threads to be had: the ones there and the caller claim every task between them)
        }
        std::function<void(int)> job = std::ref(f);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &job;
            njobs_ = n;
            next_.store(0, std::memory_order_relaxed);
            pending_ = n;
            ++gen_;
        }
        cv_start_.notify_all();
        const int finished = claim(job, n);
        std::unique_lock<std::mutex> lk(mu_);
        pending_ -= finished;
        // (a worker that took this section's job may not have claimed from the counter yet: the section ends only when it
        // has left too — else the next section's reset counter would hand it an index it checks against this n)
        cv_done_.wait(lk, [this]() { return pending_ == 0 && active_ == 0; });
        job_ = nullptr;
    }

  private:
    int claim(const std::function<void(int)> &job, int n) {
        int finished = 0;
        for (;;) {
            const int i = next_.fetch_add(1, std::memory_order_relaxed);
            if (i >= n) return finished;
            job(i);
            ++finished;
        }
    }
    void worker() {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(int)> *job = nullptr;
            int n = 0;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_start_.wait(lk, [&]() { return stop_ || (gen_ != seen && job_ != nullptr); });
                if (stop_) return;
                seen = gen_;
                job = job_;
                n = njobs_;
                ++active_;
            }
            const int finished = claim(*job, n);
            std::lock_guard<std::mutex> lk(mu_);
            pending_ -= finished;
            --active_;
            if (pending_ == 0 && active_ == 0) cv_done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_start_, cv_done_;
    const std::function<void(int)> *job_ = nullptr;
    std::atomic<int> next_{0};
    int njobs_ = 0, pending_ = 0, active_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

template <class F>
static void parallel_for(int n, F &&f) {
    static thread_local WorkPool pool;
    pool.run(n, std::forward<F>(f));
}
