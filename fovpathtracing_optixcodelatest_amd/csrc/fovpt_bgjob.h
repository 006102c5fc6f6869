// fovpt_bgjob.h -- one background job slot and its state machine (FOVPT_UPDATE_REBUILD_ASYNC, include/fovpt.h).  Host only and
// free of HIP: the job itself is a callable the user supplies, so tests/cpp/bgjob_test.cpp drives this header with a fake build
// under the thread and address sanitizers.
//
//   request   IDLE: the job starts on a thread of its own (BUILDING); BUILDING or READY: ignored.  Counted either way.
//   finished  the job returned 0: READY, its result waits to be adopted.
//   failed    the job returned a code: IDLE again, the code and the job's text are kept (last_error, last_text), nothing else.
//   adopt     READY: the result goes to the caller, IDLE.  Otherwise nothing.
//   discard   joins a running job; a result, adopted by nobody, goes to the caller's `drop`.  IDLE.  (The destructor discards.)
//
// Every member function is called from ONE thread, the owner's.  The job's thread touches nothing but the result, the text and
// the flag it publishes them with (a release store; the owner reads it with acquire, or joins), so the owner sees the finished
// state only when it asks: in state(), wait(), adopt() or discard().
#pragma once
#include <atomic>
#include <cstdint>
#include <functional>
#include <string>
#include <thread>
#include <utility>

namespace fovpt {

template <class Result> class BgJob {
public:
    enum State { IDLE = 0, BUILDING = 1, READY = 2 };                  // FOVPT_REBUILD_IDLE / _BUILDING / _READY
    using Build = std::function<int(Result&, std::string&)>;           // on the job's thread: 0 and the result, or a code and its text
    using Drop = std::function<void(Result&)>;                         // on the owner's thread: frees a result nobody adopts
    struct Counters { uint64_t requested = 0, started = 0, adopted = 0, failed = 0, discarded = 0; };

    BgJob() = default;
    BgJob(const BgJob&) = delete;
    BgJob& operator=(const BgJob&) = delete;
    ~BgJob() { discard(drop_); }

    // what frees a result that is still here when the slot goes away
    void on_destroy(Drop d) { drop_ = std::move(d); }

    // true: the job started.  false: one is running or its result waits (the request is counted and otherwise ignored)
    bool request(Build build)
    {
        counters_.requested++;
        if (state() != IDLE) return false;
        counters_.started++;
        done_.store(0, std::memory_order_relaxed);
        result_ = Result();
        text_.clear();
        slot_ = BUILDING;
        thread_ = std::thread([this, build] {
            const int rc = build(result_, text_);
            code_ = rc;
            done_.store(1, std::memory_order_release);
        });
        return true;
    }

    // a request that the owner found nothing to start for (it looked at state() earlier in the same call): counted, as request() counts it
    void count_ignored() { counters_.requested++; }

    // READY: the result that waits (it stays); otherwise null
    const Result* peek() { return state() == READY ? &result_ : nullptr; }

    // never blocks
    State state()
    {
        if (slot_ == BUILDING && done_.load(std::memory_order_acquire)) finish();
        return slot_;
    }

    // blocks while BUILDING, and for nothing else
    State wait()
    {
        if (slot_ == BUILDING) finish();
        return slot_;
    }

    // READY: *out takes the result
    bool adopt(Result* out)
    {
        if (state() != READY) return false;
        *out = std::move(result_);
        result_ = Result();
        slot_ = IDLE;
        counters_.adopted++;
        return true;
    }

    // true: a job was running or a result waited.  A result goes to `drop`; a job that failed meanwhile counts as failed.
    bool discard(const Drop& drop)
    {
        if (wait() != READY) return false;
        if (drop) drop(result_);
        result_ = Result();
        slot_ = IDLE;
        counters_.discarded++;
        return true;
    }

    const Counters& counters() const { return counters_; }
    int last_error() const { return last_error_; }                     // 0, or the code of the last job that failed
    const std::string& last_text() const { return last_text_; }

private:
    // the job's thread has published, or is about to: join it and take what it left
    void finish()
    {
        thread_.join();
        if (code_ == 0) { slot_ = READY; return; }
        slot_ = IDLE;
        counters_.failed++;
        last_error_ = code_;
        last_text_ = text_;
        result_ = Result();
    }

    State slot_ = IDLE;
    std::thread thread_;
    std::atomic<int> done_{0};
    int code_ = 0;                 // (written by the job's thread ahead of done_)
    Result result_{};
    std::string text_;
    Counters counters_;
    int last_error_ = 0;
    std::string last_text_;
    Drop drop_;
};

}  // namespace fovpt
