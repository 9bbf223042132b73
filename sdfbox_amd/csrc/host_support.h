// What the host side of libsdfhip.so shares beyond the scene handle: the HIP_TRY prefix form, growable buffers, the builders' arenas,
// and the call frame of the calls that build a tree on the device (NoMem, AllocFault, DeviceBuffers, CallStream, finish_tree, and
// CallFrame, which holds them for edit.hip, prune.hip, combine.hip, place.hip, compose.hip, volume.hip, distance.hip and blend.hip;
// trigen.hip brings arenas of its own to the same parts).  Not one of the renderer's measured sources (bench_report.py
// hashes scene.h, which this header includes and which must never include it): a helper a new translation unit needs goes here.
#pragma once
#include "scene.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

// HIP_TRY (scene.h) with a translation unit's prefix in front of the message.  Used through one-line aliases that pass #expr as
// `text`, so that the message shows the call as it was written: #define M_TRY(expr) HIP_TRY_AS("multi: ", expr, #expr)
#define HIP_TRY_AS(prefix, expr, text)                                                      \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) {                                                             \
            (void)hipGetLastError();   /* the runtime's record of it: a later launch check must not report it as its own */ \
            return sdfhip::fail(SDFHIP_ERR_DEVICE, prefix "%s failed: %s", text, hipGetErrorString(e_)); \
        }                                                                                   \
    } while (0)

namespace sdfhip {

#if defined(__x86_64__) || defined(__i386__)
inline void cpu_relax() { __builtin_ia32_pause(); }      // inside a spin loop
#else
inline void cpu_relax() { std::this_thread::yield(); }
#endif

// The camera block as a march reads it: render.hip's unpack_info, field for field (the same IEEE operations, once per call on the
// host), for the translation units outside the renderer's measured sources (query.hip, instances.hip)
inline void unpack_camera(const sdfhip_info *in, FrameInfo &I)
{
    memset(&I, 0, sizeof I);
    I.h0x = in->heading[0][0]; I.h0y = in->heading[0][1]; I.h0z = in->heading[0][2];
    I.h1x = in->heading[1][0]; I.h1y = in->heading[1][1]; I.h1z = in->heading[1][2];
    I.h2x = in->heading[2][0]; I.h2y = in->heading[2][1]; I.h2z = in->heading[2][2];
    I.posx = in->position[0]; I.posy = in->position[1]; I.posz = in->position[2];
    I.margin = in->margin;
    I.margin2 = in->margin * 2.0f;
    I.screen_w = in->screen_size[0]; I.screen_h = in->screen_size[1];
    I.limit = in->limit;
    I.lightx = in->light[0]; I.lighty = in->light[1]; I.lightz = in->light[2];
    I.fov = in->fov;
    I.k_strength = exp2f(in->strength) - 1.0f;
    I.half_aspect = in->screen_size[0] / in->screen_size[1] * 0.5f;
}

// A buffer on the current device that grows on demand; its owner keeps the pointer and the capacity in bytes.
// grow_buffer: room for `need` bytes (the contents are not kept).  drain: a stream whose work may still use the old block, waited
// for before that is freed.  The caller words a failure: *failed (when given) names the call that returned it; after a failed
// allocation the buffer is empty.  release_buffer: frees a block larger than `keep` bytes.
template <class T> void release_buffer(T *&p, size_t &cap, size_t keep = 0)
{
    if (cap > keep) { (void)hipFree(p); p = nullptr; cap = 0; }
}
template <class T> hipError_t grow_buffer(T *&p, size_t &cap, size_t need, hipStream_t drain = nullptr, const char **failed = nullptr)
{
    if (need <= cap) return hipSuccess;
    if (failed) *failed = "hipStreamSynchronize(drain)";
    hipError_t e = drain ? hipStreamSynchronize(drain) : hipSuccess;
    if (e != hipSuccess) return e;
    release_buffer(p, cap);
    if (failed) *failed = "device_alloc((void **)p, need)";
    e = device_alloc(&p, need);
    if (e != hipSuccess) p = nullptr; else cap = need;
    return e;
}

// The finished tree (n nodes, 8 bytes of each array per node) from device memory into two host arrays from alloc(bytes), which
// the library's caller frees with free().  On failure nothing is left allocated, `out` is untouched and the runtime's record is
// cleared; *no_host_memory (when given) tells an allocation that failed from a copy that did.
template <class Alloc>
hipError_t tree_to_host(const void *d_structs, const void *d_values, size_t n, Alloc alloc, sdfhip_octdata *out, bool *no_host_memory = nullptr)
{
    int32_t *S = static_cast<int32_t *>(alloc(n * 8));
    uint8_t *V = static_cast<uint8_t *>(alloc(n * 8));
    if (no_host_memory) *no_host_memory = !(S && V);
    hipError_t e = !(S && V) ? hipErrorOutOfMemory : hipMemcpy(S, d_structs, n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(V, d_values, n * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { (void)hipGetLastError(); free(S); free(V); return e; }
    out->length = (uint32_t)n; out->structs = S; out->values = V;
    return hipSuccess;
}

// device_memory.hip: the pool the builder's arenas take their chunks from and give them back to (device_alloc_bytes trims it when
// the device is out of memory).  pool_take: a chunk of `want` bytes or somewhat more, its size in *size; null when the pool
// holds none (or SDFHIP_GEN_POOL=0).
void *pool_take(int device, size_t want, size_t *size);
void pool_give(int device, void *base, size_t size);

// The builders' device memory (sdfgen_device.hip, trigen.hip).  Bump allocator over a few large hipMalloc chunks.  reset() makes the memory reusable; work on
// the (single, in-order) stream that still reads the old contents was launched before whatever
// is launched to overwrite them, so no synchronisation is needed.  The chunks outlive a build: they come from and go back to the
// per-process pool of device_memory.hip.
struct Arena {
    struct Chunk { char *base; size_t size, used; };
    std::vector<Chunk> chunks;
    size_t grow;
    int device = 0;
    explicit Arena(size_t grow) : grow(grow) { (void)hipGetDevice(&device); }
    Arena(const Arena &) = delete;
    Arena &operator=(const Arena &) = delete;
    void *take(size_t bytes)
    {
        bytes = (bytes + 255) & ~(size_t)255;
        if (bytes == 0) bytes = 256;
        for (auto &c : chunks)
            if (c.size - c.used >= bytes) { void *p = c.base + c.used; c.used += bytes; return p; }
        size_t size = bytes > grow ? bytes : grow;
        void *p = pool_take(device, size, &size);
        if (!p) {
            const auto t0 = std::chrono::steady_clock::now();
            // (device_alloc_bytes: the pool may be holding what this allocation needs, in chunks of other sizes)
            if (device_alloc_bytes(&p, size) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
            const float ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (ms > 5.0f && lab_env("SDFHIP_GEN_LEVELS")) fprintf(stderr, "sdfgen: hipMalloc(%zu MB) took %.1f ms\n", size >> 20, ms);
        }
        chunks.push_back(Chunk{ (char *)p, size, bytes });
        grow = grow < ((size_t)1 << 30) ? grow * 2 : grow;
        return p;
    }
    template <class T> T *alloc(size_t n) { return (T *)take(n * sizeof(T)); }
    void reset() { for (auto &c : chunks) c.used = 0; }
    ~Arena() { for (auto &c : chunks) pool_give(device, c.base, c.size); }
};

// ---- the call frame of the calls that turn a tree on the device into a new scene (CallFrame's users, trigen.hip) -----------------

constexpr int TREE_MAX_DEPTH = 12;          // LM: the deepest tree the grids and the cursor-stack kernels take

// blocks of 256 threads for a grid-stride loop over `threads` items
inline dim3 grid_stride_blocks(uint64_t threads, uint32_t cap = 4096) { return dim3((uint32_t)std::min<uint64_t>((threads + 255) / 256, cap)); }

// Thrown by a call's allocator; the entry point catches it and words its SDFHIP_ERR_NOMEM.
struct NoMem {};

// laboratory library: VARIABLE=k fails the call's k-th allocation (0 = the first), once.  The product reads nothing (lab_env).
struct AllocFault {
    int left = -1;
    explicit AllocFault(const char *variable) { if (const char *e = lab_env(variable)) left = atoi(e); }
    bool next()                                     // is this allocation the one to fail?
    {
        if (left == 0) { left = -1; return true; }
        if (left > 0) left--;
        return false;
    }
};

// A call's device memory: grown on demand, freed at the end (the arrays the scene is made from included: it keeps its own copy)
struct DeviceBuffers {
    std::vector<void *> owned;
    AllocFault fault;
    explicit DeviceBuffers(const char *fault_variable) : fault(fault_variable) {}
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;
    ~DeviceBuffers() { for (void *p : owned) (void)hipFree(p); }
    template <class T> T *get(size_t count)
    {
        void *p = nullptr;
        if (fault.next()) throw NoMem{};
        const hipError_t e = device_alloc_bytes(&p, count ? count * sizeof(T) : 1);
        if (e != hipSuccess) { (void)hipGetLastError(); throw NoMem{}; }
        owned.push_back(p);
        return static_cast<T *>(p);
    }
    void drop(void *p)
    {
        for (auto &q : owned)
            if (q == p) { (void)hipFree(q); q = owned.back(); owned.pop_back(); return; }
    }
    // a buffer of at least `need` elements (contents not kept)
    template <class T> void ensure(T *&p, size_t &cap, size_t need)
    {
        if (need <= cap) return;
        if (p) drop(p);
        p = nullptr;
        cap = need + need / 2;
        p = get<T>(cap);
    }
};

// A call's own non-blocking stream and N timing events.  The destructor waits for the stream before it destroys anything, so it
// is declared after the call's memory (CallFrame's members; trigen.hip's arenas): the stream must be drained before the memory its
// kernels use is freed (or goes back to the pool) on whatever path the call returns.
template <int N> struct CallStream {
    hipStream_t st = nullptr;
    hipEvent_t ev[N] = {};
    CallStream() = default;
    CallStream(const CallStream &) = delete;
    CallStream &operator=(const CallStream &) = delete;
    // what: the translation unit's HIP_TRY_AS prefix ("" for plain HIP_TRY)
    int open(const char *what)
    {
        const auto tried = [what](hipError_t e, const char *text) {
            if (e == hipSuccess) return (int)SDFHIP_OK;
            (void)hipGetLastError();
            return fail(SDFHIP_ERR_DEVICE, "%s%s failed: %s", what, text, hipGetErrorString(e));
        };
        if (const int rc = tried(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreateWithFlags(&st, hipStreamNonBlocking)")) return rc;
        for (int k = 0; k < N; k++)
            if (const int rc = tried(hipEventCreate(&ev[k]), "hipEventCreate(&ev[k])")) return rc;
        return SDFHIP_OK;
    }
    ~CallStream()
    {
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
        for (int k = 0; k < N; k++) if (ev[k]) (void)hipEventDestroy(ev[k]);
    }
};

// The rewriters' shared tail: the finished arrays (n nodes, `depth` levels deep by construction) as a scene handle when `scene` is
// given, and as host arrays (malloc) when `host_out` is.  If the copy to the host fails the new scene is freed and *scene stays
// as it was.  *scene_ms: the host's time for the handle.
inline int finish_tree(const char *what, int device, const int2 *dS, const uint2 *dV, uint32_t n, int depth, sdfhip_scene **scene,
                       sdfhip_octdata *host_out, float *scene_ms)
{
    const auto t0 = std::chrono::steady_clock::now();
    sdfhip_scene *res = nullptr;
    if (scene) {
        const int rc = scene_from_arrays(device, reinterpret_cast<const int32_t *>(dS), reinterpret_cast<const uint8_t *>(dV), n, true, nullptr,
                                         &res, depth);
        if (rc != SDFHIP_OK) return rc;
    }
    *scene_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (host_out) {
        bool no_host_memory = false;
        const hipError_t e = tree_to_host(dS, dV, n, malloc, host_out, &no_host_memory);
        if (e != hipSuccess) {
            if (res) (void)sdfhip_scene_free(res);
            return no_host_memory ? fail(SDFHIP_ERR_NOMEM, "%s: out of host memory for host_out", what)
                                  : fail(SDFHIP_ERR_DEVICE, "%s: copying the tree to the host failed: %s", what, hipGetErrorString(e));
        }
    }
    if (scene) *scene = res;
    return SDFHIP_OK;
}

// What a call that builds on `device` holds from its last refusal on, once: what: the entry point's name as its messages begin;
// fault_variable: DeviceBuffers'; t0: the call's first line.  The members in this order: whichever way the call returns, the
// stream is drained, then the buffers are freed, then the caller's device is restored.
template <int N> struct CallFrame {
    const char *what;
    int device;
    std::chrono::steady_clock::time_point t0;
    DeviceGuard guard;
    DeviceBuffers bufs;
    CallStream<N> cs;
    CallFrame(const char *what, int device, const char *fault_variable, std::chrono::steady_clock::time_point t0 = {})
        : what(what), device(device), t0(t0), guard(device), bufs(fault_variable) {}
    // Opens the stream and runs body(stream), the call's passes.  untouched: what a call that ran out of memory says it has left
    // as it was ("the source is untouched").
    template <class Body> int run(const char *untouched, Body body)
    try {
        if (!guard.ok) return (void)hipGetLastError(), fail(SDFHIP_ERR_DEVICE, "%s: hipSetDevice(%d) failed", what, device);
        if (const int rc = cs.open("")) return rc;
        return body(cs.st);
    } catch (const NoMem &) {
        return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory (%s)", what, untouched);
    }
    // the time between two of the call's events, both recorded and reached
    int elapsed(float *ms, int from, int to) const { HIP_TRY(hipEventElapsedTime(ms, cs.ev[from], cs.ev[to])); return SDFHIP_OK; }
    int finish(const int2 *dS, const uint2 *dV, uint32_t n, int depth, sdfhip_scene **scene, sdfhip_octdata *host_out, float *scene_ms) const
    {
        return finish_tree(what, device, dS, dV, n, depth, scene, host_out, scene_ms);
    }
    float total_ms() const { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- the passes over a scene's cells that return no tree: mesh.hip, slice.hip, measure.hip ("The cell pass") ----

// (the texts below print TREE_MAX_DEPTH where the cell passes' own checks printed cell_tets.h's MESH_MAX_DEPTH: both are LM)
static_assert(TREE_MAX_DEPTH == LM, "one depth limit: cell_tets.h's MESH_MAX_DEPTH is LM too");
constexpr int MAX_DEVICES = 64;                     // (query.hip keeps a constant of this name and value for its staging buffers)
constexpr size_t HEAD_BYTES = 256;                  // a pass's header (its totals and counts), in front of what it keeps per chunk
constexpr size_t KEEP_BYTES = (size_t)16 << 20;     // a block up to this size stays allocated between calls

// what every call on the surface's cells refuses of a level and of a handle; none: "no mesh", "no slice", "no measure"
inline int check_level(const char *what, int32_t level)
{
    if (level < -1 || level > TREE_MAX_DEPTH) return fail(SDFHIP_ERR_ARG, "%s: level %d is neither -1 nor 0..%d", what, level, TREE_MAX_DEPTH);
    return SDFHIP_OK;
}
inline int check_cell_scene(const char *what, const sdfhip_scene *s, const char *none)
{
    if (!s->stack_ok || s->depth > (uint32_t)TREE_MAX_DEPTH)
        return fail(SDFHIP_ERR_BAD_TREE, "%s: the tree is not consistent (or deeper than %d levels): %s", what, TREE_MAX_DEPTH, none);
    if (s->device < 0 || s->device >= MAX_DEVICES) return fail(SDFHIP_ERR_ARG, "%s: device %d", what, s->device);
    return SDFHIP_OK;
}

// A feature's temporaries on one device: a header of HEAD_BYTES and the per-chunk array behind it.  They cannot live in the scene
// handle (scene.h belongs to the renderer's measured sources), so each feature keeps an array of these, one per device, and a call
// holds `lock` (before the handle's) from its first use to release().  An emit may be left in flight on the caller's stream: the
// next call waits for it through `busy`, the library's own event, never through that stream, before it writes the block again.
// (A synchronous user such as the measure never emits: begin() creates its `busy` too, and it stays unused.)
struct DeviceScratch {
    std::mutex lock;
    char *buf = nullptr;
    size_t cap = 0;
    hipEvent_t busy = nullptr, ev0 = nullptr, ev1 = nullptr;
    bool pending = false;                           // an emit that reads buf may be in flight: `busy` is behind it

    template <class H> H *head() { return reinterpret_cast<H *>(buf); }
    template <class T> T *behind_head() { return reinterpret_cast<T *>(buf + HEAD_BYTES); }

    // The block idle, `need` bytes large and its header zeroed on `st`.  of: what the out-of-memory refusal says the bytes are for.
    int begin(const char *what, AllocFault &fault, size_t need, const char *of, hipStream_t st)
    {
        if (!busy) HIP_TRY(hipEventCreateWithFlags(&busy, hipEventDisableTiming));       // each on its own: one may fail and the next call tries again
        if (!ev0) HIP_TRY(hipEventCreate(&ev0));
        if (!ev1) HIP_TRY(hipEventCreate(&ev1));
        if (pending) { HIP_TRY(hipEventSynchronize(busy)); pending = false; }
        if (fault.next() || grow_buffer(buf, cap, need) != hipSuccess) {
            (void)hipGetLastError();
            return fail(SDFHIP_ERR_NOMEM, "%s: out of device memory for %zu bytes of %s", what, need, of);
        }
        HIP_TRY(hipMemsetAsync(buf, 0, HEAD_BYTES, st));
        return SDFHIP_OK;
    }
    // launch(): the kernels that fill the header, on `st`.  When this returns they have run and *h is the header; *ms (when given)
    // is their time.
    template <class H, class Launch> int count(hipStream_t st, Launch launch, H *h, float *ms)
    {
        static_assert(sizeof(H) <= HEAD_BYTES, "the header's room in front of the per-chunk array");
        if (ms) HIP_TRY(hipEventRecord(ev0, st));
        launch();
        HIP_TRY(hipGetLastError());
        if (ms) HIP_TRY(hipEventRecord(ev1, st));
        HIP_TRY(hipMemcpyAsync(h, buf, sizeof(H), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ms) HIP_TRY(hipEventElapsedTime(ms, ev0, ev1));
        return SDFHIP_OK;
    }
    // launch(): the kernel that reads the block and writes the output, left in flight on `st`; the block stays busy until it has run
    template <class Launch> int emit(hipStream_t st, Launch launch)
    {
        launch();
        pending = true;                             // (whatever the launch said: the wait is harmless)
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(busy, st));
        return SDFHIP_OK;
    }
    // ... the same, then copy_out() -- the copies to the host, on `st` -- and the wait: nothing is in flight; *ms: the emit's time
    template <class Launch, class Copy> int emit_to_host(hipStream_t st, Launch launch, Copy copy_out, float *ms)
    {
        HIP_TRY(hipEventRecord(ev0, st));
        if (const int rc = emit(st, launch)) return rc;
        HIP_TRY(hipEventRecord(ev1, st));
        if (const int rc = copy_out()) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        pending = false;
        HIP_TRY(hipEventElapsedTime(ms, ev0, ev1));
        return SDFHIP_OK;
    }
    // A call that frees buffers of its own (the host forms) settles first: nothing of it is in flight on `st` when they go, however
    // it ended.  Every call ends with release(): the block goes when it is idle and above KEEP_BYTES.
    void settle(hipStream_t st) { if (pending) { (void)hipStreamSynchronize(st); pending = false; } }
    void release() { if (!pending) release_buffer(buf, cap, KEEP_BYTES); }
};

}  // namespace sdfhip
