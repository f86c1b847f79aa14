// fd_host_pool.h — a context's host helper threads.  No device and no HIP call: host C++ alone (fdgpu_internal.h and fd_match_tables.h include it).
#pragma once
#include <stdint.h>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// A context's host helper threads (the per-candidate glue of whole-structure retrievals, fd_host_query.hip): started once, woken per job — spawning
// nineteen std::threads per pass cost ~1 ms of a 10 ms retrieval.  run(n, f): f() on n - 1 pool threads and on the caller, returns when all are done.
struct fd_host_pool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv, cv_done;
    const std::function<void()> *job = nullptr;
    uint64_t gen = 0;
    unsigned want = 0, taken = 0, active = 0;
    bool stop = false;
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void()> *f = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || (gen != seen && taken < want); });
                if (stop) return;
                seen = gen; ++taken; f = job;
            }
            (*f)();
            {
                std::lock_guard<std::mutex> lk(mu);
                --active;
            }
            cv_done.notify_one();
        }
    }
    void run(unsigned n, const std::function<void()> &f) {
        if (n <= 1) { f(); return; }
        const unsigned helpers = n - 1;
        {
            std::lock_guard<std::mutex> lk(mu);
            while (th.size() < helpers) th.emplace_back([this] { loop(); });
            job = &f; want = helpers; taken = 0; active = helpers; ++gen;
        }
        cv.notify_all();
        f();
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return active == 0; });
        job = nullptr;
    }
    ~fd_host_pool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        for (auto &t : th) t.join();
    }
};
