// sr_trace: the host-array entry point, and the pipeline that takes a large bundle through in chunks.  Host code only -- no
// kernel is launched from this file: it drives the public sr_rays_* / sr_stream_select entries and sr::download_rows (trace.hip).
//
// A large bundle goes through in chunks that alternate between the library's two streams, so that the upload of chunk i+1 and
// the download of chunk i-1 (host-synchronous copies of pageable memory) run while chunk i is traced (the traces themselves one
// after the other: see `serial` below).  Rays are independent and every output row is written at its own rays' columns: the
// arrays are those of the single pass, bit for bit.  No hipMalloc / hipFree inside the loop after the first two chunks
// (hipFree waits for every stream).
#include <sys/mman.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#include "common.hpp"

namespace {

// The environment switches of one sr_trace call, read once per call.
struct PipelineKnobs {
  // SYNTHRAY_TRACE_CHUNK: most rays per chunk; 0 = never pipeline.  Default 2.5 * 2^20: 1e7 rays in four chunks of 2.5e6, dense
  // enough for the tile path's records kernel (15 rays per cell of a 4 mm beam on 512^3) -- 77.7 ms per call with page-locked
  // result arrays; 2^20: 79.5, 1.5 * 2^20: 84 (chunks at the tile path's threshold, where it is no faster than the per-ray
  // kernel), 2^21: 80, 3.4e6: 77.7, 5e6: 80.5 (profiles/r05_pcie_host_arrays.txt)
  int64_t chunk = (int64_t)5 << 19;
  bool cache = true;  // SYNTHRAY_TRACE_CACHE=0: the device side of the pipeline is not kept between calls
  // The chunks' TRACES run one after the other, each behind the one before (an event wait; the streams still alternate, so
  // the download of chunk i runs beside the trace of chunk i+1): two traces side by side finish together, and the first one's
  // download then overlaps nothing -- 104 -> 91 ms per 1e7 rays at 2^21-ray chunks, 119 -> 104 at 5e6.  SYNTHRAY_TRACE_SERIAL=0:
  // side by side, as before.
  bool serial = true;
  bool debug = false;  // SYNTHRAY_TRACE_DEBUG: where the caller's thread spends its time, chunk by chunk, on stderr
};
PipelineKnobs pipeline_knobs() {
  PipelineKnobs k;
  if (const char *e = getenv("SYNTHRAY_TRACE_CHUNK")) k.chunk = atoll(e);
  if (const char *e = getenv("SYNTHRAY_TRACE_CACHE")) k.cache = e[0] != '0';
  if (const char *e = getenv("SYNTHRAY_TRACE_SERIAL")) k.serial = atoi(e) != 0;
  k.debug = getenv("SYNTHRAY_TRACE_DEBUG") != nullptr;
  return k;
}

// Result arrays that are ordinary (pageable, never written) NumPy memory cost a page fault per 4 KB when the copy engine's
// staging thread first writes them: 1.36 GB of sf / rf / Jf for 1e7 rays, more time than the trace.  MADV_POPULATE_WRITE
// maps the pages WITHOUT touching their contents (safe beside copies already landing), and several threads do it side by
// side while the first chunks are uploaded and traced.  Page-locked arrays (sr_host_alloc) are left alone.
void populate_pages(double *p, size_t bytes, std::vector<std::thread> &pool) {
  if (!p || bytes < ((size_t)8 << 20)) return;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type != hipMemoryTypeUnregistered) return;  // page-locked already
  (void)hipGetLastError();
  const uintptr_t page = 4096, lo = ((uintptr_t)p + page - 1) & ~(page - 1), hi = ((uintptr_t)p + bytes) & ~(page - 1);
  if (hi <= lo) return;
  const int n_thr = 4;
  const uintptr_t per = (((hi - lo) / n_thr) + page - 1) & ~(page - 1);
  for (int t = 0; t < n_thr; ++t) {
    const uintptr_t a = lo + (uintptr_t)t * per, b = std::min(hi, a + per);
    if (a < b) pool.emplace_back([a, b]() { (void)madvise((void *)a, b - a, 23 /* MADV_POPULATE_WRITE */); });
  }
}

constexpr int kRing = 3;  // bundles in flight: one being traced on each of the two streams, one being uploaded

// The device side of the pipeline -- three chunk-sized ray bundles and two staging blocks, ~2.5 GB of HBM at the default
// chunk -- is KEPT between calls (a loop of solve() calls: ~40 hipMalloc + ~40 hipFree, each of which waits for the device,
// were 6 of a call's 85 ms).  Released by sr_release_caches(), by a call with another chunk size or device, and not kept at
// all with SYNTHRAY_TRACE_CACHE=0.  A call works on the cached set in place and releases it when it fails: whole set or nothing.
struct PipelineCache {
  int64_t chunk = 0;
  int device = -1;
  sr_rays *ring[kRing] = {nullptr, nullptr, nullptr};
  double *staging[2] = {nullptr, nullptr};
} g_pipe;
void release_pipeline_cache() {
  for (auto &r : g_pipe.ring) {
    if (r) sr_rays_destroy(r);
    r = nullptr;
  }
  for (auto &q : g_pipe.staging) {
    sr::dev_free(q);
    q = nullptr;
  }
  g_pipe.chunk = 0;
  g_pipe.device = -1;
}

// Page-locked bounce buffers of the library's own (two chunks' worth, allocated at the first large sr_trace and kept): the
// runtime's copy from pageable memory runs on ONE thread at ~8 GB/s -- 90 ms for the 0.72 GB of 1e7 rays, more than their
// trace; four threads copying into a page-locked buffer and a DMA from there move them in a quarter of that.
double *g_bounce[2] = {nullptr, nullptr};
size_t g_bounce_rays = 0;
bool ensure_bounce(int64_t cap) {
  if (g_bounce_rays < (size_t)cap) {
    for (auto &b : g_bounce) {
      if (b) (void)hipHostFree(b);
      b = nullptr;
    }
    g_bounce_rays = 0;
    if (hipHostMalloc(reinterpret_cast<void **>(&g_bounce[0]), sizeof(double) * 9 * (size_t)cap, hipHostMallocDefault) == hipSuccess &&
        hipHostMalloc(reinterpret_cast<void **>(&g_bounce[1]), sizeof(double) * 9 * (size_t)cap, hipHostMallocDefault) == hipSuccess)
      g_bounce_rays = (size_t)cap;
    else
      (void)hipGetLastError();  // no page-locked memory to be had: the runtime's own staging does (slower)
  }
  return g_bounce_rays >= (size_t)cap;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// One pipelined call: what the caller's thread (trace_chunk, finish) and the uploader thread (upload_all) share.
struct Pipeline {
  const sr_volume *v;
  const double *s0;
  int64_t N;
  const sr_trace_params *p;
  double *sf, *rf, *Jf;
  PipelineKnobs knobs;
  int64_t n_chunks = 0, chunk = 0, last = 0;  // n_chunks - 1 chunks of `chunk` rays and one of `last`
  bool use_bounce = false;
  // events: uploaded[ci] (recorded by the uploader on its own stream), traced[ci] (recorded after chunk ci's trace)
  std::vector<hipEvent_t> uploaded, traced;
  // per chunk: the launch positions' bounding box (min x, y, z, max x, y, z), written by the uploader's copier threads before the
  // chunk is announced (n_uploaded, under the mutex); lo > hi: not known
  std::vector<std::array<double, 6>> boxes;
  std::mutex mu;
  std::condition_variable cv;
  int64_t n_uploaded = 0, n_traced = 0;  // chunks whose `uploaded` / `traced` event has been RECORDED (guarded by mu)
  bool abort_upload = false;
  hipError_t up_err = hipSuccess;
  sr_trace_stats tot{0, 0, 0.0, 0.0};
  int64_t prev = -1;  // the chunk whose trace is queued and whose rows are still to be copied out
  double t_begin = 0.0;

  int64_t first_ray(int64_t ci) const { return ci * chunk; }
  int64_t rays_of(int64_t ci) const { return ci + 1 < n_chunks ? chunk : last; }

  // rows [q0, q1) of chunk ci into the bounce buffer.  The three position rows are read for their bounding box while they are
  // copied (the chunk's rays per lateral cell of the BEAM choose its kernel, as for a bundle uploaded whole: trace.hip, tile_plan);
  // NaN positions compare false and are left out
  void copy_rows(int64_t ci, double *bb, int q0, int q1) {
    const int64_t off = first_ray(ci), n = rays_of(ci);
    for (int q = q0; q < q1; ++q) {
      const double *src = s0 + (size_t)q * N + off;
      double *dst = bb + (size_t)q * n;
      if (q < 3) {
        double lo = __builtin_inf(), hi = -__builtin_inf();
        for (int64_t t = 0; t < n; ++t) {
          const double x = src[t];
          dst[t] = x;
          lo = x < lo ? x : lo;
          hi = x > hi ? x : hi;
        }
        boxes[(size_t)ci][q] = lo;
        boxes[(size_t)ci][3 + q] = hi;
      } else {
        memcpy(dst, src, sizeof(double) * (size_t)n);
      }
    }
  }

  // chunk ci's rays into its bundle on the uploader's stream `us`, then uploaded[ci]
  hipError_t upload_chunk(int64_t ci, hipStream_t us, hipEvent_t (&bounce_free)[2]) {
    hipError_t e = hipSuccess;
    sr_rays *r = g_pipe.ring[ci % kRing];
    const int64_t off = first_ray(ci), n = rays_of(ci);
    if (use_bounce) {
      double *bb = g_bounce[ci & 1];
      if (ci >= 2) e = hipEventSynchronize(bounce_free[ci & 1]);  // the DMA that last read this buffer
      std::thread copiers[3];
      copiers[0] = std::thread(&Pipeline::copy_rows, this, ci, bb, 2, 4);
      copiers[1] = std::thread(&Pipeline::copy_rows, this, ci, bb, 4, 6);
      copiers[2] = std::thread(&Pipeline::copy_rows, this, ci, bb, 6, 9);
      copy_rows(ci, bb, 0, 2);
      for (auto &t : copiers) t.join();
      if (e == hipSuccess) e = hipMemcpyAsync(r->s0, bb, sizeof(double) * 9 * (size_t)n, hipMemcpyHostToDevice, us);  // rows at pitch n
      if (e == hipSuccess) e = hipEventRecord(bounce_free[ci & 1], us);
    } else {
      for (int q = 0; q < 9 && e == hipSuccess; ++q)  // rows of n rays at pitch n: a shorter last chunk uses the front of a full-size bundle
        e = hipMemcpyAsync(r->s0 + (size_t)q * n, s0 + (size_t)q * N + off, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, us);
    }
    if (e == hipSuccess) e = hipEventRecord(uploaded[ci], us);
    return e;
  }

  // The uploader: a host thread of its own, because a copy FROM pageable memory holds the thread that asked for it
  // (staged through the runtime's bounce buffers at ~15 GB/s): on the caller's thread every chunk's upload delayed the
  // download of the chunk before it and the launch of the chunk after it.
  void upload_all() {
    hipStream_t us = nullptr;
    hipError_t e = hipSetDevice(g_pipe.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&us, hipStreamNonBlocking);
    hipEvent_t bounce_free[2] = {nullptr, nullptr};
    for (auto &b : bounce_free)
      if (e == hipSuccess) e = hipEventCreateWithFlags(&b, hipEventDisableTiming);
    for (int64_t ci = 0; ci < n_chunks && e == hipSuccess; ++ci) {
      if (ci >= kRing) {  // the bundle is free again once the trace that read it is done
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return abort_upload || n_traced > ci - kRing; });
          if (abort_upload) break;
        }
        e = hipEventSynchronize(traced[ci - kRing]);
        if (e != hipSuccess) break;
      }
      e = upload_chunk(ci, us, bounce_free);
      {
        std::lock_guard<std::mutex> lk(mu);
        if (e == hipSuccess) n_uploaded = ci + 1;
      }
      cv.notify_all();
    }
    if (us) {
      (void)hipStreamSynchronize(us);
      (void)hipStreamDestroy(us);
    }
    for (auto &b : bounce_free)
      if (b) (void)hipEventDestroy(b);
    {
      std::lock_guard<std::mutex> lk(mu);
      up_err = e;
      if (e != hipSuccess) abort_upload = true;
    }
    cv.notify_all();
  }

  // waits for chunk ci's trace (its stream), copies its rows out, adds its totals
  int finish(int64_t ci) {
    sr_rays *r = g_pipe.ring[ci % kRing];
    int e = sr_stream_select((int)(ci & 1));
    if (!e) e = sr::download_rows(r, sf, rf, Jf, N, first_ray(ci), g_pipe.staging[ci & 1]);
    sr_trace_stats st{0, 0, 0.0, 0.0};
    if (!e) e = sr_rays_trace_stats(r, &st);
    tot.ray_steps += st.ray_steps;
    tot.fallback_rays += st.fallback_rays;
    tot.trace_kernel_ms += st.trace_kernel_ms;
    tot.total_ms += st.total_ms;
    return e;
  }

  // The caller's thread, chunk ci: wait for its upload, queue its trace on stream ci & 1, then finish the chunk before it
  // (on the other stream) while this one is traced.
  int trace_chunk(int64_t ci) {
    int rc = sr_stream_select((int)(ci & 1));
    if (rc) return rc;
    sr::Context &c = sr::ctx();
    const double t_a = now_ms();
    {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return abort_upload || n_uploaded > ci; });
      if (abort_upload) return sr::fail(SR_ERR_HIP, "sr_trace: upload of rays %lld..: %s", (long long)first_ray(ci), hipGetErrorString(up_err));
    }
    sr_rays *r = g_pipe.ring[ci % kRing];
    if (hipStreamWaitEvent(c.stream, uploaded[ci], 0) != hipSuccess ||
        (knobs.serial && ci > 0 && hipStreamWaitEvent(c.stream, traced[ci - 1], 0) != hipSuccess))
      return sr::fail(SR_ERR_HIP, "sr_trace: hipStreamWaitEvent failed");
    r->n = rays_of(ci);    // a shorter last chunk: the front of a full-size bundle (its rows were uploaded at pitch n)
    r->have_bbox = true;   // found by the uploader's copier threads while they copied the position rows
    for (int q = 0; q < 6; ++q) r->bbox[q] = boxes[(size_t)ci][q];
    for (int q = 0; q < 3; ++q)
      if (!(r->bbox[q] <= r->bbox[3 + q])) r->have_bbox = false;  // no bounce buffers (the runtime staged the rows), or every position NaN
    r->have_s0 = true;
    r->traced = false;
    rc = sr_rays_trace(r, v, p, nullptr);  // queued; returns at once
    if (!rc && hipEventRecord(traced[ci], c.stream) != hipSuccess) rc = sr::fail(SR_ERR_HIP, "sr_trace: hipEventRecord failed");
    {
      std::lock_guard<std::mutex> lk(mu);
      n_traced = ci + 1;
    }
    cv.notify_all();
    if (rc) return rc;
    const double t_b = now_ms();
    if (prev >= 0) rc = finish(prev);
    if (knobs.debug)
      fprintf(stderr, "sr_trace chunk %lld: at %.1f ms waited %.1f ms for its upload, queued in %.1f ms, finish(prev) %.1f ms\n", (long long)ci,
              t_a - t_begin, t_b - t_a, 0.0, now_ms() - t_b);
    prev = ci;
    return rc;
  }
};

int trace_pipelined(const sr_volume *v, const double *s0, int64_t N, const sr_trace_params *p, double *sf, double *rf, double *Jf,
                    sr_trace_stats *stats, const PipelineKnobs &knobs) {
  sr::Context &c = sr::ctx();
  const int saved = c.current;
  Pipeline P{v, s0, N, p, sf, rf, Jf, knobs};
  // `cap`: the most rays of a chunk (what the bundles, staging blocks and bounce buffers are sized for, and what the cache is
  // kept by); the chunks themselves are EQUAL parts of this call's rays -- 1e7 rays: 4 x 2.5e6, not 3 x 2.62e6 and a rest at a
  // lower ray density (the density chooses the kernel)
  const int64_t cap = knobs.chunk;
  P.n_chunks = std::max<int64_t>(2, (N + cap - 1) / cap);
  P.chunk = std::min(cap, (N + P.n_chunks - 1) / P.n_chunks);
  if ((P.n_chunks - 1) * P.chunk >= N) P.chunk = cap;  // (only chunks of a few rays: n_chunks^2 > N)
  P.last = N - (P.n_chunks - 1) * P.chunk;
  int rc = SR_OK;
  std::vector<std::thread> faulters;
  populate_pages(sf, sizeof(double) * 9 * (size_t)N, faulters);
  populate_pages(rf, sizeof(double) * 4 * (size_t)N, faulters);
  populate_pages(Jf, sizeof(double) * 4 * (size_t)N, faulters);
  // ---- set-up: bundles and staging blocks from the cache (whole set or nothing) or new, events, bounce buffers, the uploader
  if (g_pipe.chunk != cap || g_pipe.device != c.device) release_pipeline_cache();
  g_pipe.chunk = cap;
  g_pipe.device = c.device;
  for (int q = 0; q < kRing && q < P.n_chunks && !rc; ++q)
    if (!g_pipe.ring[q]) rc = sr_rays_create(&g_pipe.ring[q], cap);  // a chunk may use part of one
  for (int q = 0; q < 2 && !rc; ++q) {
    rc = sr_stream_select(q);
    if (!rc && !g_pipe.staging[q]) rc = sr::dev_alloc(&g_pipe.staging[q], (size_t)17 * (size_t)cap);
  }
  P.uploaded.assign((size_t)P.n_chunks, nullptr);
  P.traced.assign((size_t)P.n_chunks, nullptr);
  P.boxes.assign((size_t)P.n_chunks, std::array<double, 6>{1, 1, 1, 0, 0, 0});
  for (int64_t ci = 0; ci < P.n_chunks && !rc; ++ci) {
    if (hipEventCreateWithFlags(&P.uploaded[ci], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&P.traced[ci], hipEventDisableTiming) != hipSuccess)
      rc = sr::fail(SR_ERR_HIP, "sr_trace: hipEventCreate failed");
  }
  if (!rc) P.use_bounce = ensure_bounce(cap);
  std::thread uploader;
  if (!rc) uploader = std::thread(&Pipeline::upload_all, &P);
  // ---- the chunks, then the last one's rows
  P.t_begin = now_ms();
  for (int64_t ci = 0; ci < P.n_chunks && !rc; ++ci) rc = P.trace_chunk(ci);
  {
    const double t_b = now_ms();
    if (!rc && P.prev >= 0) rc = P.finish(P.prev);
    if (knobs.debug) fprintf(stderr, "sr_trace last finish at %.1f ms: %.1f ms\n", t_b - P.t_begin, now_ms() - t_b);
  }
  // ---- tear-down
  {
    std::lock_guard<std::mutex> lk(P.mu);
    if (rc) P.abort_upload = true;
  }
  P.cv.notify_all();
  if (uploader.joinable()) uploader.join();
  for (auto &t : faulters) t.join();
  (void)sr_synchronize();
  for (sr_rays *r : g_pipe.ring)
    if (r) r->n = cap;
  if (!knobs.cache || rc) release_pipeline_cache();  // else kept for the next call
  for (auto *events : {&P.uploaded, &P.traced})
    for (hipEvent_t e : *events)
      if (e) (void)hipEventDestroy(e);
  (void)sr_stream_select(saved);
  if (stats) *stats = P.tot;
  return rc;
}

}  // namespace

extern "C" {

int sr_release_caches(void) {
  if (sr::ctx().stream) (void)sr_synchronize();
  release_pipeline_cache();
  sr::scratch_release();
  return SR_OK;
}

int sr_trace(const sr_volume *v, const double *s0, int64_t n_rays, const sr_trace_params *p, double *sf, double *rf,
             double *Jf, sr_trace_stats *stats) {
  SR_CHECK(v && s0 && p, "sr_trace: NULL argument");
  const PipelineKnobs knobs = pipeline_knobs();
  const int64_t chunk = knobs.chunk;
  // from 1.2 chunks' worth of rays: two equal chunks (3.1e6 rays and more at the default, as before the chunks grew)
  if (chunk > 0 && n_rays >= chunk + chunk / 5 && n_rays >= 2 && !p->handoff) return trace_pipelined(v, s0, n_rays, p, sf, rf, Jf, stats, knobs);
  sr_rays *r = nullptr;
  int rc = sr_rays_create(&r, n_rays);
  if (rc) return rc;
  rc = sr_rays_upload(r, s0);
  if (!rc) rc = sr_rays_trace(r, v, p, stats);
  if (!rc) rc = sr_rays_download(r, sf, rf, Jf);
  sr_rays_destroy(r);
  return rc;
}

}  // extern "C"
