// Stand-alone check of the device-memory groups (vds_mem.h) for `make hostcheck`: the raw allocator is malloc / free, so the address
// sanitizer sees a block that leaks, is freed twice or is touched after it went back.  Built without VDS_CANARY / VDS_DIRTY: nothing
// here reaches the HIP runtime.  The expected choices of the recycling rule are worked out from the rule (smallest parked block of
// at least the bytes asked for and at most asked + asked / 2 + 65536, the first among equals), not from what the code does.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

static int g_raw_calls = 0, g_fail_at = -1;          // the g_fail_at-th raw allocation from now on fails (-1: none)
static hipError_t check_malloc(void **p, size_t bytes) {
    if (g_fail_at >= 0 && g_raw_calls++ == g_fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = malloc(bytes);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
static hipError_t check_free(void *p) { free(p); return hipSuccess; }
#define VDS_RAW_MALLOC(pp, bytes) check_malloc((pp), (bytes))
#define VDS_RAW_FREE(p) check_free(p)
#include "vds_mem.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "mem_check: %s fails (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static long long live() { return g_dev_blocks.load(); }
static long long live_bytes() { return g_dev_bytes.load(); }
static char *take(DevGroup &g, size_t bytes) {
    char *p = nullptr;
    CHECK(g.alloc(&p, bytes) == hipSuccess && p);
    for (size_t i = 0; i < bytes; i += 4096) p[i] = 1;          // (the block is there and ours)
    return p;
}

int main() {
    {   // ---- the recycling rule
        DevGroup g;
        g.recycle = true;
        const size_t A = 100000;                  // asked + asked / 2 + 65536 = 215536
        // parked, in this order: 215537 (one byte too large), 215536 (the largest that fits), 300000, 100000 (exact), 150000, 150000
        char *big1 = take(g, 215537), *lim = take(g, 215536), *huge = take(g, 300000), *exact = take(g, A), *mid_a = take(g, 150000), *mid_b = take(g, 150000);
        CHECK(live() == 6 && live_bytes() == 215537 + 215536 + 300000 + 100000 + 150000 + 150000);
        g.park();
        CHECK(g.empty() && live() == 6);          // parked blocks stay live
        CHECK(take(g, A) == exact);               // exact fit: the smallest of several that fit
        CHECK(take(g, A) == mid_a);               // 150000 twice: the first of two equal
        CHECK(take(g, A) == mid_b);
        CHECK(take(g, A) == lim);                 // asked + asked / 2 + 65536: taken
        CHECK(live() == 6);
        char *fresh = take(g, A);                 // one byte more and 300000: not taken - nothing fits, a fresh block
        CHECK(fresh != big1 && fresh != huge && live() == 7);
        CHECK(live_bytes() == 215537 + 215536 + 300000 + 100000 + 150000 + 150000 + 100000);      // a recycled block keeps its parked size
        CHECK(take(g, 215537) == big1 && live() == 7);
        g.drop_parked();                          // the load ends: the leftover (300000) is freed
        CHECK(live() == 6 && g.blocks.size() == 6 && g.parked.empty());
        lim[215535] = 2; fresh[A - 1] = 2;        // (what the group holds is still there)
        // a group that does not recycle frees at once
        DevGroup plain;
        take(plain, 1000);
        plain.park();
        CHECK(plain.empty() && plain.parked.empty() && live() == 6);
    }       // (the group's end frees the rest)
    CHECK(live() == 0 && live_bytes() == 0);
    {   // ---- one block out of the middle; clearing twice
        DevGroup g;
        char *a = take(g, 64), *b = take(g, 128), *c = take(g, 256);
        g.release(b);
        CHECK(live() == 2 && live_bytes() == 64 + 256 && g.blocks.size() == 2 && g.blocks[0].p == a && g.blocks[1].p == c);
        a[63] = 3; c[255] = 3;
        g.release(b);                             // not of this group any more: nothing
        g.release(nullptr);
        CHECK(live() == 2);
        g.clear();
        g.clear();
        CHECK(live() == 0 && g.empty());
        take(g, 32);                              // and it can be used again
        g.release_all();
        g.release_all();
        CHECK(live() == 0 && live_bytes() == 0);
    }
    {   // ---- the k-th raw allocation fails: nothing leaks, the group stays usable
        for (int k = 0; k < 4; ++k) {
            DevGroup g;
            g_raw_calls = 0; g_fail_at = k;
            int got = 0;
            for (int i = 0; i < 4; ++i) {
                int *p = (int *)16;
                const hipError_t e = g.alloc(&p, (size_t)100 + i);
                CHECK((e == hipSuccess) == (i != k) && (e == hipSuccess ? p != nullptr : p == nullptr));
                if (e == hipSuccess) { p[99 + i] = 4; ++got; }
            }
            g_fail_at = -1;
            CHECK(got == 3 && live() == 3 && (int)g.blocks.size() == 3 && live_bytes() == (long long)sizeof(int) * (100 + 101 + 102 + 103 - (100 + k)));
            take(g, 8);
            CHECK(live() == 4);
        }
        CHECK(live() == 0 && live_bytes() == 0);
    }
    {   // ---- 0 elements gives 1
        DevGroup g;
        long long *p = nullptr;
        CHECK(g.alloc(&p, 0) == hipSuccess && p && live() == 1 && live_bytes() == (long long)sizeof(long long) && g.blocks[0].bytes == sizeof(long long));
        *p = 5;
    }
    CHECK(live() == 0 && live_bytes() == 0);
    puts("mem_check: ok");
    return 0;
}
