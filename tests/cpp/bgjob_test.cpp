// bgjob_test.cpp -- the state machine of FOVPT_UPDATE_REBUILD_ASYNC (csrc/fovpt_bgjob.h) with a fake build: no HIP, no device.
// Built by tests/test_rebuild_async_cpu.py with -fsanitize=thread and again with -fsanitize=address,undefined; exit status 0
// and no sanitizer report is the test.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <thread>

#include "fovpt_bgjob.h"

namespace {

// what a fake build yields: heap memory somebody has to free exactly once (the address sanitizer reports a leak or a double free)
struct Tree { int* nodes = nullptr; int value = 0; };
using Job = fovpt::BgJob<Tree>;

int g_dropped = 0;
void drop(Tree& t) { delete[] t.nodes; t.nodes = nullptr; g_dropped++; }

#define REQUIRE(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

// a build that takes `ms`, then yields `value`, or fails with `code`
Job::Build fake(int ms, int value, int code = 0)
{
    return [=](Tree& out, std::string& text) {
        if (ms) std::this_thread::sleep_for(std::chrono::milliseconds(ms));
        if (code) { text = "fake build failed"; return code; }
        out.nodes = new int[16];
        out.nodes[0] = value;
        out.value = value;
        return 0;
    };
}

void test_request_finished_adopt()
{
    Job j;
    j.on_destroy(drop);
    REQUIRE(j.state() == Job::IDLE);
    Tree t;
    REQUIRE(!j.adopt(&t));                              // nothing to adopt on IDLE
    REQUIRE(j.request(fake(20, 7)));
    REQUIRE(j.state() == Job::BUILDING);
    REQUIRE(!j.adopt(&t));                              // nor on BUILDING
    REQUIRE(j.wait() == Job::READY);
    REQUIRE(j.state() == Job::READY);
    REQUIRE(j.adopt(&t) && t.value == 7 && t.nodes && t.nodes[0] == 7);
    REQUIRE(j.state() == Job::IDLE);
    REQUIRE(!j.adopt(&t));
    drop(t);
    const Job::Counters& c = j.counters();
    REQUIRE(c.requested == 1 && c.started == 1 && c.adopted == 1 && c.failed == 0 && c.discarded == 0 && j.last_error() == 0);
}

void test_requests_ignored_and_counted()
{
    Job j;
    j.on_destroy(drop);
    REQUIRE(j.request(fake(30, 1)));
    REQUIRE(!j.request(fake(0, 2)));                    // while BUILDING
    REQUIRE(j.counters().requested == 2 && j.counters().started == 1);
    REQUIRE(j.wait() == Job::READY);
    REQUIRE(!j.request(fake(0, 3)));                    // while READY
    REQUIRE(j.counters().requested == 3 && j.counters().started == 1);
    Tree t;
    REQUIRE(j.adopt(&t) && t.value == 1);               // the first build's result, not a later request's
    drop(t);
    REQUIRE(j.request(fake(0, 4)));                     // IDLE again: a new one starts
    REQUIRE(j.wait() == Job::READY && j.adopt(&t) && t.value == 4);
    drop(t);
    REQUIRE(j.counters().requested == 4 && j.counters().started == 2 && j.counters().adopted == 2);
}

void test_failed_then_new_request()
{
    Job j;
    j.on_destroy(drop);
    REQUIRE(j.request(fake(5, 0, -6)));
    REQUIRE(j.wait() == Job::IDLE);                     // a failed build keeps nothing
    REQUIRE(j.counters().failed == 1 && j.last_error() == -6 && j.last_text() == "fake build failed");
    Tree t;
    REQUIRE(!j.adopt(&t));
    REQUIRE(j.request(fake(0, 9)));
    REQUIRE(j.wait() == Job::READY && j.adopt(&t) && t.value == 9);
    drop(t);
    REQUIRE(j.last_error() == -6);                      // the last build that failed
    REQUIRE(j.counters().started == 2 && j.counters().failed == 1 && j.counters().adopted == 1);
}

void test_discard_and_join()
{
    const int before = g_dropped;
    Job j;
    j.on_destroy(drop);
    REQUIRE(!j.discard(drop));                          // IDLE: nothing to discard
    REQUIRE(j.request(fake(40, 5)));
    REQUIRE(j.discard(drop));                           // still running: joined, its result dropped
    REQUIRE(g_dropped == before + 1 && j.state() == Job::IDLE && j.counters().discarded == 1);
    REQUIRE(j.request(fake(0, 6)));
    REQUIRE(j.wait() == Job::READY);
    REQUIRE(j.discard(drop));                           // READY: dropped too
    REQUIRE(g_dropped == before + 2 && j.counters().discarded == 2);
    REQUIRE(j.request(fake(10, 0, -3)));
    REQUIRE(!j.discard(drop));                          // a build that fails while it is joined is a failed build
    REQUIRE(j.counters().failed == 1 && j.counters().discarded == 2 && j.state() == Job::IDLE);
}

void test_destruction_while_running()
{
    const int before = g_dropped;
    {
        Job j;
        j.on_destroy(drop);
        REQUIRE(j.request(fake(40, 8)));
    }
    REQUIRE(g_dropped == before + 1);
    {
        Job j;
        j.on_destroy(drop);
        REQUIRE(j.request(fake(0, 8)));
        REQUIRE(j.wait() == Job::READY);
    }
    REQUIRE(g_dropped == before + 2);
}

void test_random_rounds()
{
    std::mt19937 rng(12345);
    auto ms = [&] { return (int)(rng() % 3); };
    Job j;
    j.on_destroy(drop);
    uint64_t started = 0, adopted = 0, failed = 0, discarded = 0, requested = 0;
    for (int round = 0; round < 400; round++) {
        const bool fails = rng() % 5 == 0;
        const bool was_idle = j.state() == Job::IDLE;
        const uint64_t failed_before = j.counters().failed;
        requested++;
        const bool began = j.request(fake(ms(), round, fails ? -6 : 0));
        REQUIRE(began == was_idle || (!was_idle && j.counters().failed > failed_before));   // (a build may fail between the two looks)
        if (began) started++;
        if (ms()) std::this_thread::sleep_for(std::chrono::milliseconds(ms()));
        switch (rng() % 4) {
        case 0: {
            Tree t;
            if (j.adopt(&t)) { adopted++; REQUIRE(t.nodes && t.nodes[0] == t.value); drop(t); }
            break;
        }
        case 1: {
            Tree t;
            j.wait();
            REQUIRE(j.state() != Job::BUILDING);
            if (j.adopt(&t)) { adopted++; drop(t); }
            break;
        }
        case 2: if (j.discard(drop)) discarded++; break;
        default: break;                                  // leave it running into the next round
        }
        failed = j.counters().failed;
    }
    j.discard(drop) ? discarded++ : 0;
    failed = j.counters().failed;
    const Job::Counters& c = j.counters();
    REQUIRE(c.requested == requested && c.started == started && c.adopted == adopted && c.discarded == discarded);
    REQUIRE(started == adopted + failed + discarded);   // every build that started ended one of three ways
}

}  // namespace

int main()
{
    test_request_finished_adopt();
    test_requests_ignored_and_counted();
    test_failed_then_new_request();
    test_discard_and_join();
    test_destruction_while_running();
    test_random_rounds();
    printf("bgjob ok\n");
    return 0;
}
