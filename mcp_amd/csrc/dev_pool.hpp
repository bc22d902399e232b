// dev_pool.hpp — the C ABI's device-side resources that outlive a call: the per-device cache
// of workspace blocks (with its MCPX_POISON debug mode) and the free list of stream pairs
// the host-buffer pipeline runs on.  Part of mcpx_api.cpp, the only file that includes it
// (hence the unnamed namespace).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace {

// Library-internal device buffers: a per-device cache of hipMalloc'd blocks, never unmapped.
// A block goes back to the cache with an event recorded on the stream of its last use; the
// next user (any stream of that device) takes it after a stream wait on that event, so reuse
// stays stream-ordered without host synchronisation.  (HIP 7.2's stream-ordered pools —
// hipMallocFromPoolAsync / hipFreeAsync, whose default VM heap remaps recycled memory — gave
// wrong answers here: from the fourth back-to-back host call on, ~15 of 1,024 T = 10 games
// every other call, with torch's bundled HIP 7.0 runtime or DEBUG_HIP_MEM_POOL_VMHEAP=0
// never; tools/band_stress.py)  Idle blocks beyond kCacheKeep bytes per
// device are freed once their last use has completed; the cache lives for the process (no
// HIP calls during teardown).
constexpr uint64_t kCacheKeep = 4ull << 30;

// MCPX_POISON=1 (debug): every block handed out is filled with 0xFF bytes (NaN doubles) up to
// the requested size, and the rest of the block (at least kCanary bytes) with the canary byte
// 0xA5.  At release the tail is read back and checked: a write past the requested size is
// reported on stderr ("MCPX_POISON canary") and counted (mcpx_debug_canary_violations), and a
// kernel result that depended on workspace read before it was written turns NaN or changes.
// Host synchronisation at every release: a diagnostic mode, not for timing.
constexpr size_t kCanary = 4096;
constexpr unsigned char kCanaryByte = 0xA5;
std::atomic<int64_t> g_canary_bad{0};

bool poison_on() {
  static const bool on = [] {
    const char* v = std::getenv("MCPX_POISON");
    return v && std::atoi(v) == 1;
  }();
  return on;
}

struct Block {
  void* p = nullptr;
  size_t bytes = 0;
  size_t req = 0;             // MCPX_POISON: the size requested by the current user
  hipEvent_t last = nullptr;  // recorded after the block's last use
  bool busy = false;
};

// MCPX_POISON: fill a block just handed out (stream-ordered)
hipError_t poison_block(Block& b, size_t bytes, hipStream_t st) {
  b.req = bytes;
  hipError_t e = hipMemsetAsync(b.p, 0xFF, bytes, st);
  if (e == hipSuccess) e = hipMemsetAsync((char*)b.p + bytes, kCanaryByte, b.bytes - bytes, st);
  return e;
}

// MCPX_POISON: check a block's tail after its last use on `st` (host-synchronising)
void check_canary(const Block& b, hipStream_t st) {
  const size_t tail = b.bytes - b.req;
  std::vector<unsigned char> h(tail);
  if (hipMemcpyAsync(h.data(), (const char*)b.p + b.req, tail, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    std::fprintf(stderr, "MCPX_POISON canary: could not read back block %p\n", b.p);
    g_canary_bad.fetch_add(1);
    return;
  }
  for (size_t i = 0; i < tail; ++i)
    if (h[i] != kCanaryByte) {
      std::fprintf(stderr, "MCPX_POISON canary: block %p (%zu bytes requested, %zu held) overwritten at +%zu\n",
                   b.p, b.req, b.bytes, b.req + i);
      g_canary_bad.fetch_add(1);
      return;
    }
}

struct BlockCache {
  std::mutex mu;
  std::map<int, std::vector<Block>> dev;  // device → blocks
  // The block at `p` and its device's list (call with `mu` held), or nullptr.
  Block* find(void* p, std::vector<Block>** list) {
    for (auto& kv : dev)
      for (auto& b : kv.second)
        if (b.p == p) {
          *list = &kv.second;
          return &b;
        }
    return nullptr;
  }
};

BlockCache& block_cache() {
  static BlockCache* c = new BlockCache;  // never destroyed
  return *c;
}

hipError_t dev_alloc(void** p, size_t bytes, hipStream_t st) {
  *p = nullptr;
  int d = 0;
  hipError_t e = hipGetDevice(&d);
  if (e != hipSuccess) return e;
  const size_t need = std::max<size_t>(bytes, 1) + (poison_on() ? kCanary : 0);
  const size_t want = (need + (2u << 20) - 1) / (2u << 20) * (2u << 20);  // 2 MiB granules
  BlockCache& c = block_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  auto& v = c.dev[d];
  Block* best = nullptr;  // the smallest idle block that fits without wasting more than half of it
  for (auto& b : v)
    if (!b.busy && b.bytes >= want && b.bytes <= 2 * want && (!best || b.bytes < best->bytes)) best = &b;
  if (best) {
    if (best->last && (e = hipStreamWaitEvent(st, best->last, 0)) != hipSuccess) return e;
    if (poison_on() && (e = poison_block(*best, bytes, st)) != hipSuccess) return e;
    best->busy = true;
    *p = best->p;
    return hipSuccess;
  }
  Block b;
  b.bytes = want;
  if ((e = hipMalloc(&b.p, want)) != hipSuccess) {
    // out of memory: free the idle blocks (after their last use) and try once more
    for (auto it = v.begin(); it != v.end();) {
      if (it->busy) { ++it; continue; }
      if (it->last) (void)hipEventSynchronize(it->last), (void)hipEventDestroy(it->last);
      (void)hipFree(it->p);
      it = v.erase(it);
    }
    (void)hipGetLastError();
    if ((e = hipMalloc(&b.p, want)) != hipSuccess) return e;
  }
  if (poison_on() && (e = poison_block(b, bytes, st)) != hipSuccess) return e;
  b.busy = true;
  v.push_back(b);
  *p = b.p;
  return hipSuccess;
}

void dev_release(void* p, hipStream_t st) {
  if (!p) return;
  BlockCache& c = block_cache();
  std::vector<Block>* list = nullptr;
  if (poison_on()) {
    // the read-back synchronises with the device, so it runs on a copy of the record and
    // without the lock: the block is still busy, nobody else takes, moves or frees it
    Block held;
    {
      std::lock_guard<std::mutex> lock(c.mu);
      const Block* b = c.find(p, &list);
      if (!b) return;
      held = *b;
    }
    check_canary(held, st);
  }
  std::lock_guard<std::mutex> lock(c.mu);
  Block* b = c.find(p, &list);
  if (!b) return;
  if (!b->last) (void)hipEventCreateWithFlags(&b->last, hipEventDisableTiming);
  if (b->last) (void)hipEventRecord(b->last, st);
  b->busy = false;
  auto& v = *list;
  uint64_t idle = 0;  // trim: idle bytes beyond kCacheKeep, oldest first, once completed
  for (auto& q : v) idle += q.busy ? 0 : q.bytes;
  for (auto it = v.begin(); it != v.end() && idle > kCacheKeep;) {
    if (it->busy || it->p == p || (it->last && hipEventQuery(it->last) != hipSuccess)) { ++it; continue; }
    idle -= it->bytes;
    if (it->last) (void)hipEventDestroy(it->last);
    (void)hipFree(it->p);
    it = v.erase(it);
  }
}

template <class T>
struct DevBuf {  // a cache block used on the null stream (synchronous callers)
  T* p = nullptr;
  ~DevBuf() { dev_release(p, nullptr); }
  hipError_t alloc(size_t count) { return count ? dev_alloc((void**)&p, count * sizeof(T), nullptr) : hipSuccess; }
};

template <class T>
struct AsyncBuf {  // a cache block, released on the stream it was allocated on
  T* p = nullptr;
  hipStream_t st = nullptr;
  hipError_t alloc(size_t count, hipStream_t s) {
    st = s;
    return count ? dev_alloc((void**)&p, count * sizeof(T), s) : hipSuccess;
  }
  ~AsyncBuf() { dev_release(p, st); }
};

// Pinned host staging for the small tables a device-buffer call builds from host metadata (the
// group lookup of mcpx_*_batch_grouped_device): the caller may free its metadata when the call
// returns, so the copy to the device runs from a buffer of the library's.  A buffer is reused once
// the event recorded after its last copy has completed; idle ones beyond kStageKeep are freed.
constexpr size_t kStageKeep = 8;
struct Stage {
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;
  bool busy = false;
};
std::mutex g_stage_mu;
std::vector<Stage> g_stages;

hipError_t stage_acquire(size_t bytes, void** p) {
  *p = nullptr;
  std::lock_guard<std::mutex> lock(g_stage_mu);
  for (auto& s : g_stages)
    if (!s.busy && s.bytes >= bytes && (!s.done || hipEventQuery(s.done) == hipSuccess)) {
      s.busy = true;
      *p = s.p;
      return hipSuccess;
    }
  (void)hipGetLastError();  // hipErrorNotReady of a query is no error of this call
  Stage s;
  s.bytes = std::max<size_t>(bytes, 4096);
  if (hipError_t e = hipHostMalloc(&s.p, s.bytes, hipHostMallocDefault); e != hipSuccess) return e;
  s.busy = true;
  g_stages.push_back(s);
  *p = s.p;
  return hipSuccess;
}

// After the last copy out of `p` was enqueued on `st`.
void stage_release(void* p, hipStream_t st) {
  if (!p) return;
  std::lock_guard<std::mutex> lock(g_stage_mu);
  size_t idle = 0;
  for (auto& s : g_stages) {
    if (s.p == p) {
      if (!s.done) (void)hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
      if (s.done) (void)hipEventRecord(s.done, st);
      s.busy = false;
    }
    idle += s.busy ? 0 : 1;
  }
  for (auto it = g_stages.begin(); it != g_stages.end() && idle > kStageKeep;) {
    if (it->busy || it->p == p || (it->done && hipEventQuery(it->done) != hipSuccess)) { ++it; continue; }
    if (it->done) (void)hipEventDestroy(it->done);
    (void)hipHostFree(it->p);
    it = g_stages.erase(it);
    --idle;
  }
  (void)hipGetLastError();
}

// The host-buffer pipeline's two streams and per-buffer events.  Creating streams per call
// maps new hardware queues every time (≈10 ms per call: profiles/r02/host_pipeline_trace.txt),
// so they come from a process-wide free list per device: a call takes one Pipe and gives
// it back when it returns, concurrent calls get different ones (the ABI stays
// reentrant), and none is ever destroyed (no HIP calls during process teardown).
constexpr int kMaxHostBufs = 8;  // most θ buffers the pipeline rotates through (MCPX_HOST_BUFFERS)
struct Pipe {
  hipStream_t up = nullptr, comp = nullptr;  // H→D uploads (serialised: full PCIe rate each), kernels
  hipEvent_t copied[kMaxHostBufs] = {}, consumed[kMaxHostBufs] = {};
  hipError_t init() {
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&up, hipStreamNonBlocking)) != hipSuccess) return e;
    if ((e = hipStreamCreateWithFlags(&comp, hipStreamNonBlocking)) != hipSuccess) return e;
    for (int k = 0; k < kMaxHostBufs; ++k) {
      if ((e = hipEventCreateWithFlags(&copied[k], hipEventDisableTiming)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&consumed[k], hipEventDisableTiming)) != hipSuccess) return e;
    }
    return hipSuccess;
  }
  void destroy() {  // a Pipe whose init() failed part-way: release what it created
    for (int k = 0; k < kMaxHostBufs; ++k) {
      if (copied[k]) (void)hipEventDestroy(copied[k]);
      if (consumed[k]) (void)hipEventDestroy(consumed[k]);
    }
    if (up) (void)hipStreamDestroy(up);
    if (comp) (void)hipStreamDestroy(comp);
  }
};

std::mutex g_pipe_mu;
std::map<int, std::vector<Pipe*>> g_pipe_free;

struct PipeLease {  // a Pipe of device `dev` for the duration of one call (current device = dev)
  Pipe* p = nullptr;
  int dev = -1;
  hipError_t acquire(int d) {
    dev = d;
    {
      std::lock_guard<std::mutex> lock(g_pipe_mu);
      auto& v = g_pipe_free[d];
      if (!v.empty()) {
        p = v.back();
        v.pop_back();
        return hipSuccess;
      }
    }
    Pipe* q = new Pipe;
    if (hipError_t e = q->init(); e != hipSuccess) {
      q->destroy();
      delete q;
      return e;
    }
    p = q;
    return hipSuccess;
  }
  ~PipeLease() {
    if (!p) return;
    std::lock_guard<std::mutex> lock(g_pipe_mu);
    g_pipe_free[dev].push_back(p);
  }
};

}  // namespace
