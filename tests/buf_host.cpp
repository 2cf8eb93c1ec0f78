// buf_host.cpp — stand-alone driver of the context's self-freeing buffers (DevBuf / PinnedBuf, csrc/bdx_ctx.h) over a stub of
// the four runtime calls they make: the stubs hand out host memory, count every call and know which pointers are live, so a
// buffer freed twice, never, or by the wrong call is seen here (and by ASan, under which tests/test_buffers_cpu.py builds this).
//   buf_host        prints `buffer driver ok: <device allocations> <device frees> <pinned allocations> <pinned frees>`
#include <set>
#include <utility>
#include <vector>

#include "bdx_ctx.h"

static std::set<void *> g_live[2];  // device, pinned
static int g_alloc[2], g_free[2], g_bad, g_fail_next;

static hipError_t stub_alloc(int kind, void **p, size_t n) {
    if (g_fail_next) {
        g_fail_next -= 1;
        return hipErrorOutOfMemory;  // (*p is left alone, as the runtime leaves it)
    }
    *p = malloc(n ? n : 1);
    g_live[kind].insert(*p);
    g_alloc[kind] += 1;
    return hipSuccess;
}
static hipError_t stub_free(int kind, void *p) {
    if (!g_live[kind].erase(p)) {
        g_bad += 1;  // freed twice, or never allocated by this call's twin
        return hipErrorInvalidValue;
    }
    g_free[kind] += 1;
    free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return stub_alloc(0, p, n); }
hipError_t hipFree(void *p) { return stub_free(0, p); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return stub_alloc(1, p, n); }
hipError_t hipHostFree(void *p) { return stub_free(1, p); }
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "buf_host.cpp:%d: %s\n", __LINE__, #c); return 1; } } while (0)

// B: the buffer type; ensure(b, bytes) grows it
template <class B, class Ensure>
static int exercise(int kind, Ensure ensure) {
    const auto live = [&]() { return (int)g_live[kind].size(); };
    const int a0 = g_alloc[kind], f0 = g_free[kind];
    {
        B a;
        CHECK(!a.p && a.cap == 0 && live() == 0);
        CHECK(ensure(a, 1000) == hipSuccess && a.p && a.cap >= 1000 && live() == 1);
        void *const first = a.p;
        CHECK(ensure(a, 500) == hipSuccess && a.p == first && g_alloc[kind] == a0 + 1);  // fits: no call
        CHECK(ensure(a, 5000) == hipSuccess && a.cap >= 5000 && live() == 1 && g_free[kind] == f0 + 1);  // grows: the old block goes, once
        B b(std::move(a));  // move construction: one owner
        CHECK(!a.p && a.cap == 0 && b.p && b.cap >= 5000 && live() == 1);
        B c;
        CHECK(ensure(c, 64) == hipSuccess && live() == 2);
        void *const moved = b.p;
        c = std::move(b);  // move assignment onto a live buffer: its own block goes, once
        CHECK(c.p == moved && !b.p && live() == 1);
        B &self = c;
        c = std::move(self);  // onto itself: nothing happens
        CHECK(c.p == moved && live() == 1);
        CHECK(ensure(a, 10) == hipSuccess && live() == 2);  // a moved-from buffer is an empty one
        a.release();
        a.release();  // (released twice: freed once)
        CHECK(!a.p && live() == 1);
        g_fail_next = 1;
        CHECK(ensure(a, 10) != hipSuccess && !a.p && a.cap == 0 && live() == 1);  // a failed allocation owns nothing
        g_fail_next = 1;
        CHECK(ensure(c, 1 << 20) != hipSuccess && !c.p && c.cap == 0 && live() == 0);  // a failed growth: the old block is gone, nothing is owned
        std::vector<B> v;  // a vector that grows moves its elements
        for (int i = 0; i < 100; ++i) {
            B e;
            CHECK(ensure(e, 256 + i) == hipSuccess);
            v.push_back(std::move(e));
            CHECK(live() == i + 1);
        }
        v.erase(v.begin() + 10, v.begin() + 20);
        CHECK(live() == 90);
        B kept = std::move(v[0]);
        v.clear();
        CHECK(live() == 1 && kept.p);
        CHECK(ensure(b, 300) == hipSuccess && live() == 2);
    }  // destruction: kept, b
    CHECK(live() == 0 && g_alloc[kind] - a0 == g_free[kind] - f0 && g_bad == 0);
    return 0;
}

int main() {
    static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf has one owner");
    static_assert(!std::is_copy_constructible<PinnedBuf>::value && !std::is_copy_assignable<PinnedBuf>::value, "PinnedBuf has one owner");
    if (exercise<DevBuf>(0, [](DevBuf &b, size_t n) { return b.ensure(n); })) return 1;
    if (exercise<PinnedBuf>(1, [](PinnedBuf &b, size_t n) { return b.ensure(n, 128); })) return 1;
    if (g_alloc[0] < 100 || g_alloc[1] < 100 || g_bad) return 1;
    printf("buffer driver ok: %d %d %d %d\n", g_alloc[0], g_free[0], g_alloc[1], g_free[1]);
    return 0;
}
