// The owner of the engine's late buffers (vil_sensor_fusion_amd/csrc/vf_device_buf.hpp) on the CPU: the four HIP calls it
// uses are the counting stubs below (the HIP runtime is not linked), so every allocation and every free is seen, a double
// free or a leak is a failure here, and one an AddressSanitizer build of this program reports as well.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "vf_device_buf.hpp"

namespace {
std::set<void*> live[2];          // blocks alive: device, pinned
int mallocs = 0, frees = 0, bad_frees = 0, fail_next = 0;
size_t last_size = 0;
hipError_t stub_malloc(int kind, void** p, size_t n) {
    if (fail_next > 0 && --fail_next == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(n ? n : 1);
    live[kind].insert(*p);
    mallocs++;
    last_size = n;
    return hipSuccess;
}
hipError_t stub_free(int kind, void* p) {
    if (!live[kind].erase(p)) { bad_frees++; return hipErrorInvalidValue; }     // freed twice, or with the other kind's call
    free(p);
    frees++;
    return hipSuccess;
}
int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { failures++; printf("FAIL line %d: %s\n", __LINE__, #cond); } \
    } while (0)
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return stub_malloc(0, p, n); }
hipError_t hipFree(void* p) { return stub_free(0, p); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) { return stub_malloc(1, p, n); }
hipError_t hipHostFree(void* p) { return stub_free(1, p); }
}

template <typename Buf>
void table(int kind) {
    const int m0 = mallocs, f0 = frees;
    {
        Buf b;
        CHECK(b.get() == nullptr && b.bytes() == 0);
        CHECK(b.ensure(0) == hipSuccess && mallocs == m0);                           // nothing asked for: nothing made
        CHECK(b.ensure(100) == hipSuccess && b.get() && b.bytes() == 100 && mallocs == m0 + 1 && last_size == 100);
        CHECK(live[kind].count(b.get()) == 1);                                       // ... by the call of its kind
        auto* first = b.get();
        ((char*)b.get())[0] = ((char*)b.get())[99] = 7;                              // (the block is there, all of it)
        CHECK(b.ensure(100) == hipSuccess && b.ensure(1) == hipSuccess && b.get() == first && mallocs == m0 + 1 && frees == f0);
        // growth: the old block freed exactly once, the new one of the head-roomed size
        CHECK(b.ensure(101, vf::twice) == hipSuccess && b.bytes() == 202 && last_size == 202 && mallocs == m0 + 2 && frees == f0 + 1);
        CHECK(b.ensure(202, vf::twice) == hipSuccess && mallocs == m0 + 2);          // within the headroom
        CHECK(b.ensure(300, [](size_t n) { return n < 4096 ? (size_t)4096 : 2 * n; }) == hipSuccess && b.bytes() == 4096 && frees == f0 + 2);
        // a failed growth: empty, size 0 -- never a freed pointer with a size -- and usable again
        fail_next = 1;
        CHECK(b.ensure(5000) == hipErrorOutOfMemory && b.get() == nullptr && b.bytes() == 0 && frees == f0 + 3 && mallocs == m0 + 3);
        CHECK(b.ensure(10) == hipSuccess && b.bytes() == 10 && mallocs == m0 + 4);
        // moves empty their source
        Buf c(std::move(b));
        CHECK(b.get() == nullptr && b.bytes() == 0 && c.bytes() == 10 && mallocs == m0 + 4 && frees == f0 + 3);
        Buf d;
        CHECK(d.ensure(20) == hipSuccess);
        auto* held = c.get();
        d = std::move(c);                                                            // d's own block goes, c's comes
        CHECK(c.get() == nullptr && c.bytes() == 0 && d.get() == held && d.bytes() == 10 && frees == f0 + 4);
        std::swap(b, d);                                                             // (what vf_engine_grow does to the arrays)
        CHECK(b.get() == held && d.get() == nullptr && frees == f0 + 4);
        Buf& same = b;
        b = std::move(same);                                                         // onto itself: nothing happens
        CHECK(b.get() == held && b.bytes() == 10 && frees == f0 + 4);
        b.release();
        CHECK(b.get() == nullptr && b.bytes() == 0 && frees == f0 + 5);
        CHECK(d.ensure(30) == hipSuccess);
    }                                                                                // destruction: d's block, once; b and c hold nothing
    CHECK(frees == f0 + 6 && mallocs == m0 + 6);
}

int main() {
    table<vf::DeviceBuf<char>>(0);
    table<vf::PinnedBuf<char>>(1);
    table<vf::DeviceBuf<double>>(0);
    CHECK(bad_frees == 0);
    CHECK(live[0].empty() && live[1].empty());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("device_buf ok\n");
    return 0;
}
