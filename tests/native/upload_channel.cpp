// The engine's upload channel and the owner of its events (vil_sensor_fusion_amd/csrc/vf_upload_channel.hpp, vf_device_buf.hpp) on
// the CPU: the HIP calls the two make are the logging stubs below (the HIP runtime is not linked), so the order of every wait, copy,
// record, allocation and free is seen.  What is expected is what vf_engine_ingest_tail, vf_engine_propagate_tail, vf_engine_gate_tail
// and the asynchronous vf_engine_preintegrate did by hand before there was a channel, written out call by call; a double free, a
// double destroy or a leak is a failure here, and one an AddressSanitizer build of this program reports as well.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <utility>

#include "vf_upload_channel.hpp"

namespace {
std::string journal;                 // the calls since the last take(), one word each
std::map<hipEvent_t, int> events;    // events alive -> e<number>, in the order they were made
std::set<void*> live[2];             // blocks alive: device, pinned
int created = 0, destroyed = 0, bad_calls = 0, fail_alloc = 0, handed_early = 0;
unsigned last_flags = 0;
char** watching = nullptr;           // where open() will put the pinned pointer: nothing there while it still waits
void say(const std::string& w) { journal += (journal.empty() ? "" : " ") + w; }
std::string take() { return std::exchange(journal, std::string()); }
std::string name(hipEvent_t ev) {
    auto it = events.find(ev);
    if (it == events.end()) { bad_calls++; return "e?"; }
    return "e" + std::to_string(it->second);
}
hipError_t stub_malloc(int kind, void** p, size_t n) {
    if (fail_alloc > 0 && --fail_alloc == 0) { *p = nullptr; say("refused"); return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    live[kind].insert(*p);
    say((kind ? "hostmalloc(" : "malloc(") + std::to_string(n) + ")");
    return hipSuccess;
}
hipError_t stub_free(int kind, void* p) {
    if (!live[kind].erase(p)) { bad_calls++; return hipErrorInvalidValue; }     // freed twice, or with the other kind's call
    free(p);
    say(kind ? "hostfree" : "free");
    return hipSuccess;
}
int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { failures++; printf("FAIL line %d: %s\n   journal: %s\n", __LINE__, #cond, journal.c_str()); } \
    } while (0)
// the journal since the last look is exactly `want`
#define SAID(want)                                                         \
    do {                                                                   \
        const std::string got_ = take();                                   \
        if (got_ != (want)) { failures++; printf("FAIL line %d:\n   want: %s\n   got:  %s\n", __LINE__, std::string(want).c_str(), got_.c_str()); } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return stub_malloc(0, p, n); }
hipError_t hipFree(void* p) { return stub_free(0, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return stub_malloc(1, p, n); }
hipError_t hipHostFree(void* p) { return stub_free(1, p); }
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned flags) {
    *ev = (hipEvent_t)malloc(1);
    events[*ev] = created++;
    last_flags = flags;
    say("create(" + name(*ev) + ")");
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
    say("destroy(" + name(ev) + ")");
    if (!events.erase(ev)) return hipErrorInvalidValue;
    free(ev);
    destroyed++;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { say("record(" + name(ev) + ")"); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t ev) {
    say("sync(" + name(ev) + ")");
    if (watching && *watching) handed_early++;
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    say("elapsed(" + name(a) + "," + name(b) + ")");
    *ms = 10.f * (events[a] % 3) + (events[b] % 3) + 0.5f;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t) {
    if (kind != hipMemcpyHostToDevice || !live[0].count(dst) || !live[1].count((void*)src)) bad_calls++;
    say("copy(" + std::to_string(n) + ")");
    return hipSuccess;
}
}

// open() as the entry points call it: the pointer arrives only after every wait
static hipError_t open(vf::UploadChannel& c, size_t bytes, char** h) {
    *h = nullptr;
    watching = h;
    const hipError_t err = c.open(bytes, h);
    watching = nullptr;
    return err;
}

// every scenario starts with no event alive: its channel's events are e<base>, e<base + 1>, e<base + 2>
static std::string e(int base, int k) { return "e" + std::to_string(base + k); }

static void timed_calls() {
    const int b = created;
    const std::string e0 = e(b, 0), e1 = e(b, 1), e2 = e(b, 2);
    {
        vf::UploadChannel c;
        char* h = nullptr;
        float t0 = -1.f, t1 = -1.f;
        CHECK(!c.outstanding() && c.device() == nullptr);
        CHECK(c.timings(&t0, &t1) == hipSuccess && t0 == 0.f && t1 == 0.f);       // before any send: zeros, no call
        SAID("");
        // the first call: three events, both blocks at twice the size, no wait
        CHECK(open(c, 100, &h) == hipSuccess && h && c.device() && live[1].count(h) && live[0].count(c.device()));
        SAID("create(" + e0 + ") create(" + e1 + ") create(" + e2 + ") hostmalloc(200) malloc(200)");
        h[0] = h[99] = 1;
        CHECK(c.send(100, nullptr, true) == hipSuccess && c.outstanding());
        SAID("record(" + e0 + ") copy(100) record(" + e1 + ")");
        t0 = t1 = -1.f;
        CHECK(c.timings(&t0, &t1) == hipSuccess && t0 == 0.f && t1 == 0.f);       // timed, no launch recorded yet: zeros, no call
        SAID("");
        CHECK(c.launched(nullptr) == hipSuccess);
        SAID("record(" + e2 + ")");
        // the next call within capacity: one wait, for the copy, before the pinned block is handed out; no allocation
        char* first = h;
        CHECK(open(c, 200, &h) == hipSuccess && h == first && handed_early == 0);
        SAID("sync(" + e1 + ")");
        // the status call of a complete send: one wait for the kernel, the two intervals
        CHECK(c.timings(&t0, &t1) == hipSuccess && t0 == 1.5f && t1 == 12.5f);
        SAID("sync(" + e2 + ") elapsed(" + e0 + "," + e1 + ") elapsed(" + e1 + "," + e2 + ")");
        CHECK(c.timings(nullptr, &t1) == hipSuccess && t1 == 12.5f);
        SAID("sync(" + e2 + ") elapsed(" + e1 + "," + e2 + ")");
        // growth with copy and kernel outstanding: the kernel's event before either block goes, then the copy's as ever
        CHECK(open(c, 500, &h) == hipSuccess && h && h != first && handed_early == 0);
        SAID("sync(" + e2 + ") hostfree hostmalloc(1000) free malloc(1000) sync(" + e1 + ")");
        h[499] = 1;
    }
    SAID("destroy(" + e2 + ") destroy(" + e1 + ") destroy(" + e0 + ") free hostfree");
}

static void untimed_calls() {
    const int b = created;
    const std::string e0 = e(b, 0), e1 = e(b, 1), e2 = e(b, 2);
    vf::UploadChannel c;
    char* h = nullptr;
    float t0 = -1.f, t1 = -1.f;
    CHECK(open(c, 10, &h) == hipSuccess);
    SAID("create(" + e0 + ") create(" + e1 + ") create(" + e2 + ") hostmalloc(20) malloc(20)");
    // growth with nothing outstanding: no wait
    CHECK(open(c, 100, &h) == hipSuccess);
    SAID("hostfree hostmalloc(200) free malloc(200)");
    // what an asynchronous preintegration sends: the copy and the event behind it, nothing else
    CHECK(c.send(100, nullptr, false) == hipSuccess && c.outstanding());
    SAID("copy(100) record(" + e1 + ")");
    CHECK(c.timings(&t0, &t1) == hipSuccess && t0 == 0.f && t1 == 0.f);
    SAID("");
    CHECK(open(c, 100, &h) == hipSuccess && handed_early == 0);
    SAID("sync(" + e1 + ")");
    // growth behind it: the copy's event is the last there is
    CHECK(open(c, 201, &h) == hipSuccess && handed_early == 0);
    SAID("sync(" + e1 + ") hostfree hostmalloc(402) free malloc(402) sync(" + e1 + ")");
    // a timed send, complete, then an untimed one: ev0 and ev2 are the earlier call's, and no interval is taken between them
    CHECK(c.send(50, nullptr, true) == hipSuccess && c.launched(nullptr) == hipSuccess && c.send(50, nullptr, false) == hipSuccess);
    take();
    t0 = t1 = -1.f;
    CHECK(c.timings(&t0, &t1) == hipSuccess && t0 == 0.f && t1 == 0.f && c.outstanding());
    SAID("");
    CHECK(open(c, 1000, &h) == hipSuccess);
    SAID("sync(" + e1 + ") hostfree hostmalloc(2000) free malloc(2000) sync(" + e1 + ")");
}

static void refused_allocation() {
    const int b = created;
    const std::string e1 = e(b, 1), e2 = e(b, 2);
    vf::UploadChannel c;
    char* h = nullptr;
    CHECK(open(c, 100, &h) == hipSuccess && c.send(100, nullptr, true) == hipSuccess && c.launched(nullptr) == hipSuccess);
    take();
    fail_alloc = 2;                                                 // the device block's turn
    CHECK(open(c, 500, &h) == hipErrorOutOfMemory && h == nullptr && c.device() == nullptr);
    SAID("sync(" + e2 + ") hostfree hostmalloc(1000) free refused");
    CHECK(open(c, 500, &h) == hipSuccess && h && c.device());      // usable again: only the block that is missing is made
    SAID("sync(" + e2 + ") malloc(1000) sync(" + e1 + ")");
    fail_alloc = 1;                                                 // the pinned block's
    CHECK(open(c, 5000, &h) == hipErrorOutOfMemory && h == nullptr);
    SAID("sync(" + e2 + ") hostfree refused");
    CHECK(open(c, 5000, &h) == hipSuccess && h && c.device());
    SAID("sync(" + e2 + ") hostmalloc(10000) free malloc(10000) sync(" + e1 + ")");
    CHECK(c.send(5000, nullptr, true) == hipSuccess);
    take();
}

static void swapped() {
    const int b = created, d0 = destroyed;
    {
        vf::UploadChannel old_arrays, grown;
        char* h = nullptr;
        float t0 = -1.f, t1 = -1.f;
        CHECK(open(old_arrays, 100, &h) == hipSuccess && old_arrays.send(100, nullptr, true) == hipSuccess && old_arrays.launched(nullptr) == hipSuccess);
        char* dev = old_arrays.device();
        take();
        std::swap(old_arrays, grown);                               // (what vf_engine_grow does to the arrays)
        SAID("");
        CHECK(grown.device() == dev && old_arrays.device() == nullptr && grown.outstanding() && !old_arrays.outstanding());
        CHECK(old_arrays.timings(&t0, &t1) == hipSuccess && t0 == 0.f && t1 == 0.f);
        SAID("");
        CHECK(grown.timings(&t0, &t1) == hipSuccess && t0 == 1.5f && t1 == 12.5f);
        SAID("sync(" + e(b, 2) + ") elapsed(" + e(b, 0) + "," + e(b, 1) + ") elapsed(" + e(b, 1) + "," + e(b, 2) + ")");
        CHECK(open(old_arrays, 10, &h) == hipSuccess);              // the emptied one starts afresh
        SAID("create(" + e(b, 3) + ") create(" + e(b, 4) + ") create(" + e(b, 5) + ") hostmalloc(20) malloc(20)");
    }
    take();
    CHECK(created == b + 6 && destroyed == d0 + 6);
}

static void event_owner() {
    const int b = created, d0 = destroyed;
    {
        vf::Event none;
        CHECK((hipEvent_t)none == nullptr);
    }
    SAID("");                                                       // an empty one: no call, made or destroyed
    {
        vf::Event a;
        CHECK(a.ensure(hipEventDisableTiming) == hipSuccess && (hipEvent_t)a != nullptr && last_flags == hipEventDisableTiming);
        CHECK(a.ensure() == hipSuccess && created == b + 1);       // there already
        hipEvent_t held = a;
        vf::Event c(std::move(a));
        CHECK((hipEvent_t)a == nullptr && (hipEvent_t)c == held);
        vf::Event d;
        CHECK(d.ensure() == hipSuccess && last_flags == hipEventDefault);
        d = std::move(c);                                           // d's own goes, c's comes
        CHECK((hipEvent_t)c == nullptr && (hipEvent_t)d == held && destroyed == d0 + 1);
        vf::Event& same = d;
        d = std::move(same);                                        // onto itself: nothing happens
        CHECK((hipEvent_t)d == held && destroyed == d0 + 1);
        std::swap(a, d);
        CHECK((hipEvent_t)a == held && (hipEvent_t)d == nullptr && destroyed == d0 + 1);
        SAID("create(" + e(b, 0) + ") create(" + e(b, 1) + ") destroy(" + e(b, 1) + ")");
    }
    SAID("destroy(" + e(b, 0) + ")");
}

int main() {
    timed_calls();
    untimed_calls();
    refused_allocation();
    swapped();
    event_owner();
    CHECK(bad_calls == 0 && handed_early == 0);
    CHECK(created == destroyed && events.empty());
    CHECK(live[0].empty() && live[1].empty());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("upload_channel ok\n");
    return 0;
}
