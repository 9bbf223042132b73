// libsdfhip.so, device memory: device_alloc_bytes -- the allocator every allocation of the scene, the render scratch, the
// multi-device handle, the edit and the queries goes through (sdfhip_internal.h) -- and the chunk pool it trims when the device is
// out of memory: the point-cloud builder's arenas (sdfgen_device.hip) keep their chunks here between builds.
#include "host_support.h"
#include "abi_guard.h"

#include <mutex>
#include <vector>

namespace {

// The arenas' chunks outlive a build: they go back to a per-process pool (by device) instead of to hipFree, and the next build
// takes them from there.  On this stack the first hipMalloc after a build had freed its ~10 GB took 340 ms -- every build after
// the first one in a process: 31 ms became 370 -- and a build's own allocations are 5 ms of it.  The pool keeps at most
// POOL_MAX_BYTES per device (what a depth-10 build of a million points needs); SDFHIP_GEN_POOL=0 turns it off.
struct ChunkPool {
    struct Item { int device; char *base; size_t size; };
    std::mutex mu;
    std::vector<Item> items;
    size_t held = 0;
    static constexpr size_t POOL_MAX_BYTES = (size_t)24 << 30;
    static bool enabled() { const char *e = getenv("SDFHIP_GEN_POOL"); return !(e && atoi(e) == 0); }
    char *take(int device, size_t want, size_t *size_out)
    {
        std::lock_guard<std::mutex> lk(mu);
        size_t best = items.size();
        for (size_t i = 0; i < items.size(); i++)        // the smallest chunk that fits, and no more than twice as large
            if (items[i].device == device && items[i].size >= want && items[i].size <= 2 * want + ((size_t)64 << 20) &&
                (best == items.size() || items[i].size < items[best].size)) best = i;
        if (best == items.size()) return nullptr;
        char *p = items[best].base;
        *size_out = items[best].size;
        held -= items[best].size;
        items.erase(items.begin() + (long)best);
        return p;
    }
    void give(int device, char *base, size_t size)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            size_t held_here = 0;                            // the limit is per device, as include/sdfhip.h says
            for (const Item &it : items) if (it.device == device) held_here += it.size;
            if (enabled() && held_here + size <= POOL_MAX_BYTES) { items.push_back(Item{device, base, size}); held += size; return; }
        }
        (void)hipFree(base);
    }
    size_t trim(int device)                              // device < 0: every device's chunks
    {
        std::vector<Item> out;
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < items.size();)
                if (device < 0 || items[i].device == device) { out.push_back(items[i]); held -= items[i].size; items.erase(items.begin() + (long)i); }
                else i++;
        }
        size_t freed = 0;
        for (auto &it : out) { (void)hipFree(it.base); freed += it.size; }
        return freed;
    }
};
ChunkPool g_pool;

}  // namespace

void *sdfhip::pool_take(int device, size_t want, size_t *size) { return ChunkPool::enabled() ? g_pool.take(device, want, size) : nullptr; }
void sdfhip::pool_give(int device, void *base, size_t size) { g_pool.give(device, static_cast<char *>(base), size); }

hipError_t sdfhip::device_alloc_bytes(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipErrorOutOfMemory) return e;
    (void)hipGetLastError();
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || g_pool.trim(device) == 0) return e;       // nothing to give back: the failure stands
    return hipMalloc(p, bytes);
}

extern "C" int sdfhip_sdfgen_trim(void)
try {
    (void)g_pool.trim(-1);
    return SDFHIP_OK;
}
SDFHIP_ABI_CATCH(sdfhip_sdfgen_trim)
