// Device memory of libvds (host code: the vds_api*.hip units through vds_handle.h, mem_check.cpp): every device block the library obtains for a handle comes from
// dev_raw_alloc and goes back through dev_free - with guard zones in the guarded build, the fill in the dirty build and the count of
// live blocks behind vds_debug_device_blocks - and belongs to exactly one DevGroup, named where it is allocated.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

// the one seam to the runtime (mem_check.cpp points it at malloc / free)
#ifndef VDS_RAW_MALLOC
#define VDS_RAW_MALLOC(pp, bytes) hipMalloc((pp), (bytes))
#define VDS_RAW_FREE(p) hipFree(p)
#endif

// Dirty build (make dirty, -DVDS_DIRTY): every byte the library obtains for a handle - device blocks from dev_raw_alloc (fresh, or a
// block of the day before out of a group's parked list), pinned staging and the blocks of PinnedPool (fresh, recycled, or ordinary
// memory) - is filled with one byte before first use: what a long-lived process gets from hipMalloc
// after it has used the memory before.  A result that depends on a table's prior content then differs from the oracle's (and
// between two fill bytes: VDS_DIRTY_FILL, a hex byte, default A5 - 0xA5A5A5A5 is a negative count, 0x5A5A5A5A a positive one).
// The fill is synchronous: nothing runs beside it.  Every other build: the two macros are empty.
#ifdef VDS_DIRTY
inline int dirty_byte() {
    static const int b = [] {
        const char *v = getenv("VDS_DIRTY_FILL");
        char *end = nullptr;
        const unsigned long x = (v && *v) ? strtoul(v, &end, 16) : 0xA5;
        return (v && *v && (*end || x > 0xFF)) ? 0xA5 : (int)x;
    }();
    return b;
}
inline void dirty_dev(void *p, size_t bytes) {
    (void)hipMemset(p, dirty_byte(), bytes);
    (void)hipDeviceSynchronize();
}
#define VDS_DIRTY_HOST(p, bytes) memset((p), dirty_byte(), (bytes))
#define VDS_DIRTY_DEV(p, bytes) dirty_dev((p), (bytes))
#else
#define VDS_DIRTY_HOST(p, bytes) ((void)0)
#define VDS_DIRTY_DEV(p, bytes) ((void)0)
#endif

// Guarded build (make canary, -DVDS_CANARY): every device table sits between two guard zones filled with a poison pattern
// (GUARD_FRONT bytes before, GUARD_BACK after).  An out-of-bounds WRITE damages a guard - vds_debug_check_guards finds it at
// the next check - and an out-of-bounds READ returns the poison (0xA5A5A5A5: a negative count / index), which the parity tests
// then see as a wrong result or a fault at a far-away address, instead of whatever the neighbouring table happened to hold.
#ifdef VDS_CANARY
static const size_t GUARD_FRONT = 64u << 10, GUARD_BACK = 256u << 10;
static const bool GUARDED = true;
#else
static const size_t GUARD_FRONT = 0, GUARD_BACK = 0;
static const bool GUARDED = false;
#endif
struct GuardRec { void *base; size_t bytes; };
inline std::map<void *, GuardRec> g_guards;      // user pointer -> allocation (guarded build only; shared by all handles and threads:
inline std::mutex g_guards_mu;                   //  every access under this lock)
inline std::atomic<long long> g_dev_blocks{0}, g_dev_bytes{0};      // live device blocks of the process and their bytes (without guards)

inline hipError_t dev_raw_alloc(void **p, size_t bytes) {
    char *base = nullptr;
    const hipError_t e = VDS_RAW_MALLOC((void **)&base, bytes + GUARD_FRONT + GUARD_BACK);
    if (e != hipSuccess) { *p = nullptr; return e; }
    if (GUARDED) {
        (void)hipMemset(base, 0xA5, GUARD_FRONT);
        (void)hipMemset(base + GUARD_FRONT + bytes, 0xA5, GUARD_BACK);
        std::lock_guard<std::mutex> lk(g_guards_mu);
        g_guards[(void *)(base + GUARD_FRONT)] = GuardRec{(void *)base, bytes};
    }
    *p = base + GUARD_FRONT;
    g_dev_blocks++; g_dev_bytes += (long long)bytes;
    VDS_DIRTY_DEV(*p, bytes);
    return hipSuccess;
}
inline void dev_free(void *p, size_t bytes) {
    if (!p) return;
    g_dev_blocks--; g_dev_bytes -= (long long)bytes;
    if (GUARDED) {
        std::lock_guard<std::mutex> lk(g_guards_mu);
        auto it = g_guards.find(p);
        if (it != g_guards.end()) { (void)VDS_RAW_FREE(it->second.base); g_guards.erase(it); return; }
    }
    (void)VDS_RAW_FREE(p);
}

// Device blocks with one lifetime.  A group with `recycle` set (the order tables: a Reload replaces ~20 tables of about the same
// size; hipFree + hipMalloc of the large ones took 1 ms or 80 ms from one call to the next: profiles/r05/load_timing_results_tables.txt)
// parks its blocks instead of freeing them (park) and hands the best fit out again: the smallest parked block (the first among equals)
// of at least the bytes asked for and at most 1.5 x + 64 KB of them; what nothing took again goes with drop_parked.  Not in the guarded
// build (a reused block's guard would not sit behind the table).
struct DevGroup {
    struct Block { void *p; size_t bytes; };
    std::vector<Block> blocks, parked;
    bool recycle = false;
    DevGroup() = default;
    DevGroup(const DevGroup &) = delete;
    DevGroup &operator=(const DevGroup &) = delete;
    ~DevGroup() { clear(); }
    bool empty() const { return blocks.empty(); }
    hipError_t alloc_bytes(void **p, size_t bytes) {
        int best = -1;
        for (int i = 0; i < (int)parked.size(); ++i) {
            const size_t cb = parked[i].bytes;
            if (cb >= bytes && cb <= bytes + bytes / 2 + 65536 && (best < 0 || cb < parked[best].bytes)) best = i;
        }
        if (best >= 0) {
            blocks.push_back(parked[best]);
            parked.erase(parked.begin() + best);
            *p = blocks.back().p;
            VDS_DIRTY_DEV(*p, blocks.back().bytes);
            return hipSuccess;
        }
        blocks.push_back(Block{nullptr, bytes});          // (before the block exists: a failed push leaks nothing)
        const hipError_t e = dev_raw_alloc(p, bytes);
        if (e != hipSuccess) blocks.pop_back();
        else blocks.back().p = *p;
        return e;
    }
    // n elements (0: one)
    template <typename T> hipError_t alloc(T **p, size_t n) { return alloc_bytes((void **)p, (n ? n : 1) * sizeof(T)); }
    void release(void *p) {                               // one block (null, or not of this group: nothing)
        for (size_t i = 0; i < blocks.size(); ++i)
            if (p && blocks[i].p == p) { dev_free(p, blocks[i].bytes); blocks.erase(blocks.begin() + i); return; }
    }
    static void free_all(std::vector<Block> &v) {
        for (const Block &b : v) dev_free(b.p, b.bytes);
        v.clear();
    }
    void release_all() { free_all(blocks); }              // the blocks in use; parked ones stay
    void park() {                                         // the blocks wait for the allocations that follow
        if (!recycle || GUARDED) { release_all(); return; }
        parked.insert(parked.end(), blocks.begin(), blocks.end());
        blocks.clear();
    }
    void drop_parked() { free_all(parked); }
    void clear() { release_all(); drop_parked(); }        // everything, the parked list included: the group's end
};
