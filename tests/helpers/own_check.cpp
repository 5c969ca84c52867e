// Stand-alone check of the host API's ownership helpers (csrc/semtsdf_own.h) over a counting fake
// allocator: malloc blocks, live blocks and bytes counted, the k-th allocation made to fail.  Four
// scripted sequences mirror the library's use (create, buffers allocated on first use, a buffer swapped
// for one of another size, scratch of one call); each runs once without a failure and once for every
// allocation position it has with that allocation failing.  A sanitizer build sees any leak, double
// free or use of a freed block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>

#include "../../slam-maskrcnn_amd/csrc/semtsdf_own.h"

static std::map<void*, size_t> g_live;
static size_t g_live_bytes = 0;
static long g_calls = 0, g_fail_at = 0, g_frees = 0, g_violations = 0;
static bool g_failed = false;

struct Fake {
    static int alloc(void** p, size_t n) {
        if (++g_calls == g_fail_at) {
            g_failed = true;
            *p = (void*)(uintptr_t)0xdead;  // a status code means: *p is not to be used
            return -3;
        }
        *p = malloc(n);
        g_live[*p] = n;
        g_live_bytes += n;
        return 0;
    }
    static void free(void* p) {
        ++g_frees;
        auto it = g_live.find(p);
        if (it == g_live.end()) {
            ++g_violations;
            printf("violation: free of a block that is not live\n");
            return;
        }
        g_live_bytes -= it->second;
        g_live.erase(it);
        ::free(p);
    }
};
using Pool = semtsdf::DevPool<Fake>;
using Scratch = semtsdf::CallScratch<Fake>;

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            ++g_violations;                                         \
            printf("violation: %s (line %d, fail_at %ld)\n", #c, __LINE__, g_fail_at); \
        }                                                           \
    } while (0)

// after every step: the pool counts exactly the live blocks (no scratch is live between steps)
static void step(const Pool& pool) { CHECK(pool.bytes() == g_live_bytes); }

// 1. semtsdf_create: allocations one after another, some of zero bytes; the first failure tears down
static void script_create() {
    const size_t sizes[] = {4096, 2048, 0, 129, 64, 0, 0, 1, 640 * 480, 16, 0, 96};
    void* ptr[sizeof(sizes) / sizeof(sizes[0])] = {};
    Pool pool;
    int rc = 0;
    for (size_t i = 0; i < sizeof(sizes) / sizeof(sizes[0]) && !rc; ++i) {
        ptr[i] = (void*)&pool;  // stale value: alloc must overwrite it
        rc = pool.alloc(&ptr[i], sizes[i]);
        CHECK(rc ? ptr[i] == nullptr : (ptr[i] != nullptr) == (sizes[i] != 0));
        if (!rc && sizes[i]) memset(ptr[i], 0xAB, sizes[i]);
        step(pool);
    }
    pool.release_all();  // free_all, on the bail path and at destroy alike
    CHECK(pool.bytes() == 0 && g_live.empty());
}

// 2. buffers allocated on first use: a pair and a single, each requested twice (a failed first request
//    leaves the whole group null, so the second one allocates)
static void script_lazy() {
    Pool pool;
    void *base = nullptr, *a = nullptr, *b = nullptr, *c = nullptr;
    if (pool.alloc(&base, 512)) return;
    step(pool);
    for (int use = 0; use < 2; ++use) {
        const size_t before = pool.bytes();
        if (!a) {
            const int rc = pool.alloc_group({{&a, 300}, {&b, 400}});
            CHECK(rc ? (!a && !b && pool.bytes() == before) : (a && b && pool.bytes() == before + 700));
            if (!rc) { memset(a, 1, 300); memset(b, 2, 400); }
        } else {
            CHECK(b != nullptr);  // never half a group
        }
        step(pool);
    }
    for (int use = 0; use < 2; ++use) {
        const size_t before = pool.bytes();
        if (!c) {
            const int rc = pool.alloc_group({{&c, 52}});
            CHECK(rc ? (!c && pool.bytes() == before) : (c && pool.bytes() == before + 52));
        }
        step(pool);
    }
    // the pool's destructor is the teardown here
}

// 3. a buffer swapped for one of another size: the fill succeeds (widen), then fails (the old array stays);
//    first from an empty slot (the tile order's first use)
static void script_swap() {
    Pool pool;
    void *slot = nullptr, *tile = nullptr;
    int rc = pool.swap(&tile, 64, [](void*) { return 0; });
    CHECK(rc ? (!tile && pool.bytes() == 0) : (tile && pool.bytes() == 64));
    step(pool);
    const size_t t = pool.bytes();
    if (pool.alloc(&slot, 100)) return;
    memset(slot, 7, 100);
    step(pool);
    void* old = slot;
    rc = pool.swap(&slot, 400, [&](void* fresh) {
        CHECK(g_live.count(old) == 1);  // the old array is there to be read while the new one is filled
        memset(fresh, *(unsigned char*)old, 400);
        return 0;
    });
    if (rc) CHECK(slot == old && pool.bytes() == t + 100 && g_live.count(old) == 1);
    else CHECK(slot != old && pool.bytes() == t + 400 && g_live.count(old) == 0 && ((unsigned char*)slot)[399] == 7);
    step(pool);
    old = slot;
    const size_t before = pool.bytes();
    rc = pool.swap(&slot, 200, [](void*) { return -2; });
    CHECK(rc != 0 && slot == old && pool.bytes() == before && g_live.count(old) == 1);
    step(pool);
    CHECK(pool.release(slot));  // still owned ...
    CHECK(!pool.release(slot));  // ... and a second release is reported, not carried out
    step(pool);
}

// 4. a call with two scratch allocations that may return between them
static int two_scratches(bool early) {
    Scratch a;
    if (int rc = a.alloc(64)) return rc;
    memset(a.get(), 0, 64);
    if (early) return 7;
    Scratch b;
    if (int rc = b.alloc(128)) return rc;
    Scratch c = std::move(b);  // the guard moves, the allocation has one owner
    memset(c.get<char>(), 0, 128);
    if (int rc = a.alloc(32)) return rc;  // a second pass of the same guard frees the first
    return 0;
}
static void script_scratch() {
    Pool pool;
    void* base = nullptr;
    if (pool.alloc(&base, 256)) return;
    for (int early = 1; early >= 0; --early) {
        const bool before = g_failed;
        const int rc = two_scratches(early);
        CHECK(rc == (g_failed != before ? -3 : early ? 7 : 0));  // the failure's status when it fell in this call
        step(pool);  // every scratch is gone, on each return path
        CHECK(g_live.size() == 1);
    }
}

// releasing what the pool does not hold
static void foreign_release() {
    Pool pool;
    void* p = nullptr;
    int on_stack = 0;
    pool.alloc(&p, 40);
    const long frees = g_frees;
    CHECK(!pool.release(&on_stack) && g_frees == frees && pool.bytes() == 40);
    CHECK(pool.release(nullptr) && g_frees == frees);
    CHECK(pool.release(p) && g_frees == frees + 1 && pool.bytes() == 0);
    CHECK(!pool.release(p) && g_frees == frees + 1);
}

static void run(const char* name, void (*script)()) {
    g_calls = g_fail_at = 0;
    g_failed = false;
    script();
    CHECK(g_live.empty() && g_live_bytes == 0);
    const long n = g_calls;
    std::string exist, visited;
    for (long k = 1; k <= n; ++k) {
        exist += (k > 1 ? "," : "") + std::to_string(k);
        g_calls = 0;
        g_fail_at = k;
        g_failed = false;
        script();
        CHECK(g_live.empty() && g_live_bytes == 0);  // after teardown: no live block
        if (g_failed) visited += (visited.empty() ? "" : ",") + std::to_string(k);
    }
    g_fail_at = 0;
    printf("script %s exist %s visited %s\n", name, exist.c_str(), visited.c_str());
}

int main() {
    run("create", script_create);
    run("lazy", script_lazy);
    run("swap", script_swap);
    run("scratch", script_scratch);
    foreign_release();
    CHECK(g_live.empty());
    printf("violations %ld\n", g_violations);
    return g_violations ? 1 : 0;
}
