// api.cpp — error plumbing shared by every entry point of libsgnrast.so, and the one-call host layer (host only).
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <hip/hip_runtime.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "sgn_common.h"

static thread_local char g_err[512] = "";

void sgn_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

SGN_EXPORT const char *sgn_last_error(void) { return g_err; }
SGN_EXPORT int sgn_version(void) { return 100; }

namespace {
int hip_fail(const char *what, hipError_t e) { sgn_set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }

// ---------------------------------------------------------------- cached events
// One untimed event per (thread, device, role), created on first use and kept: a resource cache like the error string
// above, not configuration.  Fork / join: entry points that fan work out to a caller-provided auxiliary stream
// (sgn_raster_bwd).  Count wait: the one host wait of a one-call forward.  The quats check has an event of its OWN: a
// deferred wait (check_quats = 2) stays correct whatever the library records in between.
enum EvRole { EV_FORK, EV_JOIN, EV_COUNT_WAIT, EV_QUATS_CHECK, EV_ROLES };
int cached_event(EvRole role, hipEvent_t *ev) {
    struct PerDevice { int dev; hipEvent_t e[EV_ROLES]; };
    static thread_local std::vector<PerDevice> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    PerDevice *d = nullptr;
    for (auto &p : cache)
        if (p.dev == dev) d = &p;
    if (!d) { cache.push_back(PerDevice{dev, {}}); d = &cache.back(); }
    if (!d->e[role] && hipEventCreateWithFlags(&d->e[role], hipEventDisableTiming) != hipSuccess) { d->e[role] = nullptr; return 2; }
    *ev = d->e[role];
    return 0;
}
}  // namespace

int sgn_fork_events(hipEvent_t *fork, hipEvent_t *join) {
    if (int rc = cached_event(EV_FORK, fork)) return rc;
    return cached_event(EV_JOIN, join) ? 3 : 0;
}

// ---------------------------------------------------------------- one C-ABI call per autograd node (round 5)
// The entries below run, behind ONE call each, a sequence the Python host otherwise drives call by call (sgn_rast/ops.py
// `_RasterizeGaussians.forward`).  Host only: they call the library's own entry points on the caller's stream and carve
// their temporaries from ONE arena.  What they share is written once: ReadBack, the arena layouts, forward_all.
namespace {
// host time spent BLOCKED in the one-call entries' waits (profiles: is a composite call's host time its launches or its
// wait for the device?); read and reset by sgn_timing_host_wait_us
thread_local double g_wait_us = 0.0;
thread_local long g_wait_n = 0;
inline double us_between(const timespec &a, const timespec &b) { return (b.tv_sec - a.tv_sec) * 1e6 + (b.tv_nsec - a.tv_nsec) * 1e-3; }

constexpr double SPIN_FALLBACK_US = 2.0e5;
#ifdef SGN_AB_EVENT_WAITS            // A/B builds only (profiles/scripts/build_variant.sh api eventwaits -DSGN_AB_EVENT_WAITS)
constexpr bool POLL_WAITS = false;   // round 5's form: an event behind the producing kernel, hipEventSynchronize
#else
constexpr bool POLL_WAITS = true;
#endif

// The device's view of a word of pinned host memory (nullptr: not mapped — the read-back falls back to a copy command).
int32_t *mapped(int32_t *pinned) {
    if (pinned == nullptr) return nullptr;
    void *d = nullptr;
    if (hipHostGetDevicePointer(&d, pinned, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (int32_t *)d;
}

// The one-word read-back every one-call entry waits for (the intersection count, a window's verdicts, the quats flag):
// a few words travel from the device into `host` and the host blocks — once — until host[flag_at] says they landed.
//   MAPPED transport (round 6): `host` is pinned memory with a device-side view (`direct`) and a kernel stores into it —
//   the producer itself, or sgn_publish_words behind it.  The host then POLLS the word instead of waiting for an event:
//   an event record is a barrier packet on the stream (a ~6 us bubble on the device timeline,
//   profiles/r05q_timeline_eager.md) and a host call, and its completion reaches the host later than the store itself.
//   COPY transport: a copy command and an event behind the producer; the wait is hipEventSynchronize.  (A mapped word
//   is waited for through the event too in the SGN_AB_EVENT_WAITS build, or when its `extra` word is not mapped.)
// A poll without the word after SPIN_FALLBACK_US drains the stream once (the cold path: a fault on the device, mapped
// writes that are not visible before completion); a mapped word still missing after the wait is fetched by a plain
// copy.  Every wait adds its blocked time to g_wait_us and counts once in g_wait_n.
struct ReadBack {
    enum Mapped { NEVER, IF_POLLED, ALWAYS };   // may the words travel through a mapped store?  (IF_POLLED: not for an event wait)
    const char *who, *what;      // error texts: "<who>: <what> read-back: ..."
    EvRole role;
    int flag_at;                 // host[flag_at] is the word the wait watches
    int32_t pending, landed;     // its "not landed" marker / its value once landed (landed == pending: any other value —
                                 // the watched word is the datum itself)
    int publish;                 // mapped: words sgn_publish_words carries before it sets the flag (-1: the producer stores itself)
    const int32_t *src = nullptr;        // the device words behind host[0, n_words): what the copy transport and the cold path copy
    int n_words = 1;
    const int32_t *extra_src = nullptr;  // one more word that rides with them (stored by the same thread, ahead of the flag)
    int32_t *extra_host = nullptr;
    // chosen by arm()
    int32_t *host = nullptr, *direct = nullptr, *extra_direct = nullptr;
    bool polled = false, cold = false;   // cold: the wait went into the plain copy (for its caller's error text)
    hipEvent_t ev = nullptr;

    ReadBack(const char *who_, const char *what_, EvRole role_, int flag_at_, int32_t pending_, int32_t landed_, int publish_)
        : who(who_), what(what_), role(role_), flag_at(flag_at_), pending(pending_), landed(landed_), publish(publish_) {}

    bool has_landed() const {
        const int32_t v = ((const volatile int32_t *)host)[flag_at];
        return landed == pending ? v != pending : v == landed;
    }
    // Arm, BEFORE the producer is queued: choose the transport and write the "not landed" marker.
    void arm(int32_t *pinned, int32_t *pageable, Mapped allow) {
        host = pinned ? pinned : pageable;
        if (!(extra_src && extra_host)) extra_src = extra_host = nullptr;
        direct = (allow == ALWAYS || (allow == IF_POLLED && POLL_WAITS)) ? mapped(pinned) : nullptr;
        extra_direct = direct ? mapped(extra_host) : nullptr;
        polled = POLL_WAITS && direct != nullptr && (!extra_host || extra_direct != nullptr);
        if (!polled) extra_direct = nullptr;
        if (direct) ((volatile int32_t *)host)[flag_at] = pending;
    }
    // Queue, BEHIND the producer: the publishing kernel, or the copy command(s) and the event.
    int queue(hipStream_t s) {
        if (polled)
            return publish < 0 ? 0 : sgn_publish_words(publish ? src : nullptr, publish, publish ? direct : nullptr,
                                                       direct + flag_at, landed, s);
        hipError_t e = hipSuccess;
        if (!direct && src) e = hipMemcpyAsync(host, src, sizeof(int32_t) * n_words, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && extra_host && !extra_direct)
            e = hipMemcpyAsync(extra_host, extra_src, sizeof(int32_t), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && cached_event(role, &ev) != 0) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipEventRecord(ev, s);
        if (e != hipSuccess) sgn_set_error("%s: %s read-back: %s", who, what, hipGetErrorString(e));
        return (int)e;
    }
    // Wait: the entry's one host sync (upstream: `.item()` on the count).
    hipError_t wait(hipStream_t s) {
        timespec a, b;
        clock_gettime(CLOCK_MONOTONIC, &a);
        hipError_t e = hipSuccess;
        if (!polled) e = hipEventSynchronize(ev);
        else for (unsigned it = 1; !has_landed(); ++it) {
            __builtin_ia32_pause();
            if ((it & 1023u) != 0) continue;
            (void)hipStreamQuery(s);          // (a runtime that batches submissions flushes on a query; a no-op otherwise)
            (void)hipGetLastError();          // hipErrorNotReady is the expected answer: not an error of the next launch
            clock_gettime(CLOCK_MONOTONIC, &b);
            if (us_between(a, b) > SPIN_FALLBACK_US) { e = hipStreamSynchronize(s); break; }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        clock_gettime(CLOCK_MONOTONIC, &b);
        g_wait_us += us_between(a, b);
        ++g_wait_n;
        if (e != hipSuccess || !direct || has_landed()) return e;
        cold = true;                          // never seen: the stream is drained, the plain copy is the safety net
        if (src) e = hipMemcpy(host, src, sizeof(int32_t) * n_words, hipMemcpyDeviceToHost);
        if (e == hipSuccess && extra_host) e = hipMemcpy(extra_host, extra_src, sizeof(int32_t), hipMemcpyDeviceToHost);
        return e;
    }
};

// The quats check's read-back.  flag_pinned is THREE words (round 6): [0] receives the stamp from a failing
// row, [1] the stamp from the projection kernel's first lane — "this launch's stores have landed where the host looks" —
// both as system-scope atomic stores, [2] "the projection kernel is COMPLETE": a one-wave kernel behind it stores the
// stamp there and the host polls that word; where an event behind a copy command does it instead, [2] is set to -stamp
// so that a deferred wait (sgn_project_check_wait) knows which of the two to use.
ReadBack quats_readback(const char *who, int32_t stamp) { return ReadBack(who, "flag", EV_QUATS_CHECK, 2, 0, stamp, 0); }
// after the wait: has the launch's "ok" stamp landed, and did a row fail?  This read-back has no plain copy to fall back
// on: a wait that does not find [1] == stamp drains the device once and, if the word is still missing, FAILS (a mapped
// write that is not visible at event completion must not read as "all quaternions passed").
int read_quat_flag(const int32_t *flag2, int32_t stamp, int32_t *bad, const char *who) {
    const volatile int32_t *f = flag2;
    if (f[1] != stamp) {
        (void)hipDeviceSynchronize();                          // cold path: never seen on this platform
        if (f[1] != stamp) {
            sgn_set_error("%s: the quats check's stamp never reached host memory (mapped pinned write not visible "
                          "at event completion): refusing to report 'normalized'", who);
            return -8;
        }
    }
    *bad = (f[0] == stamp) ? 1 : 0;
    return 0;
}

// ---- small shared pieces
int views_args(const char *fn, int n_views, int n) {
    if (n_views < 1 || n_views > SGN_VIEWS_MAX) {
        sgn_set_error("%s: n_views %d outside [1, %d]", fn, n_views, SGN_VIEWS_MAX);
        return -1;
    }
    if (!sgn_views_rows_ok(n_views, n)) {
        sgn_set_error("%s: n %d: need n >= 0 and n_views * n < 2^28", fn, n);
        return -2;
    }
    return 0;
}
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
sgn_raster_opts opts_or_default(const sgn_raster_opts *opts) {
    sgn_raster_opts o;
    sgn_raster_default_opts(&o);
    return opts ? *opts : o;
}
struct TileGrid { int x, y, n; };
TileGrid tile_grid(int img_h, int img_w, int block_width) {
    const int x = (img_w + block_width - 1) / block_width, y = (img_h + block_width - 1) / block_width;
    return TileGrid{x, y, x * y};
}
// forward lists with at least this many entries get four waves in the packed forward (16x16 tiles; 0: no such prefix)
int fwd_long_thresh(const sgn_raster_opts &o, int block_width) {
    return block_width == 16 ? (o.adapt_fwd > 0 ? o.adapt_fwd : 1024) : 0;
}
// An arena's layout, written once: carving with base = nullptr yields the byte size alone.
struct Carver {
    char *base;
    size_t off = 0;
    void *take(size_t bytes) { void *p = base ? base + off : nullptr; off += al256(bytes); return p; }
};
struct ForwardArena {            // sgn_rasterize_fwd_all / sgn_rasterize_views_fwd_all over `rows` rows
    int32_t *cum_r, *gid;
    float *bin_recs, *repeat;    // repeat: one more float per row (the batched entry's per-row opacities), or nullptr
    void *ws1, *ws2;
    size_t ws1_bytes, ws2_bytes, bytes;
    ForwardArena(void *base, int rows, int64_t isect_capacity, bool repeat_block) {
        const size_t nn = (size_t)(rows > 0 ? rows : 1);
        Carver c{(char *)base};
        cum_r = (int32_t *)c.take(nn * 4);
        gid = (int32_t *)c.take(nn * 4);
        bin_recs = (float *)c.take(nn * 32);
        ws1 = c.take(ws1_bytes = sgn_bin_prepare_workspace_bytes(rows));
        ws2 = c.take(ws2_bytes = sgn_bin_intersect_workspace_bytes(isect_capacity));
        repeat = repeat_block ? (float *)c.take(nn * 4) : nullptr;
        bytes = c.off + 256;
    }
};
struct WindowArena {             // sgn_rasterize_window_all
    int32_t *mismatch;
    void *lw_ws;
    size_t lw_bytes, bytes;
    WindowArena(void *base, int n_tiles) {
        Carver c{(char *)base};
        mismatch = (int32_t *)c.take(256);
        lw_ws = c.take(lw_bytes = sgn_list_window_workspace_bytes(n_tiles));
        bytes = c.off + 256;
    }
};
}  // namespace

// sgn_project_fwd_all: `project_gaussians` as ONE call — upstream's quats assertion rides the projection kernel (the
// quaternion is in its registers anyway; a failing row stamps the flag), the flag travels to the host while the depth
// ranking of the coming binning is already queued, and the host waits for it last (the "eager" check of sgn_rast/ops.py,
// which otherwise takes three calls and two more launches).  `flag_stamp` > 0: the caller guarantees that *flag_dev holds
// no value >= flag_stamp (a word zeroed ONCE and a call counter): nothing is cleared; <= 0: the call clears the flag.
// flag_pinned: quats_readback above.
SGN_EXPORT
int sgn_project_fwd_all(int n, const float *means3d, const float *scales, float glob_scale, const float *quats,
                        const float *viewmat12, float fx, float fy, float cx, float cy, int img_h, int img_w,
                        int block_width, float clip_thresh, float *cov3d, float *xys, float *depths, int32_t *radii,
                        float *conics, float *compensation, int32_t *num_tiles_hit, int check_quats, float quat_tol,
                        int32_t *flag_dev, int32_t flag_stamp, int32_t *flag_pinned, int32_t *gid_by_rank,
                        void *rank_ws, size_t rank_ws_bytes, int sort_rank_mode, int32_t *quats_bad_host,
                        int semantics, sgn_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    int32_t pageable[2] = {0, 0};
    const int32_t stamp = flag_stamp > 0 ? flag_stamp : 1;
    ReadBack rb = quats_readback("sgn_project_fwd_all", stamp);
    if (check_quats) {
        const int mode = check_quats;
        if (mode != 1 && mode != 2) { sgn_set_error("sgn_project_fwd_all: check_quats must be 0, 1 or 2"); return -3; }
        if ((!flag_dev && !(flag_stamp > 0 && flag_pinned)) || (mode == 1 && !quats_bad_host) || (mode == 2 && !flag_pinned)) { sgn_set_error("sgn_project_fwd_all: check_quats needs flag_dev and quats_bad_host (1) / flag_pinned (2)"); return -1; }
        if (flag_stamp <= 0) {
            if (!flag_dev) { sgn_set_error("sgn_project_fwd_all: flag_stamp <= 0 needs flag_dev"); return -1; }
            const hipError_t e = hipMemsetAsync(flag_dev, 0, sizeof(int32_t), s);
            if (e != hipSuccess) return hip_fail("sgn_project_fwd_all: flag clear", e);
        }
        // flag_pinned mapped into the device's address space and stamped (flag_stamp > 0: stale slots never equal the
        // stamp): a failing row stores straight into it and the read-back needs no copy command behind the kernel
        rb.arm(flag_pinned, pageable, (flag_stamp > 0 && n > 0) ? ReadBack::ALWAYS : ReadBack::NEVER);
    }
    int rc = sgn_project_fwd_checked(n, means3d, scales, glob_scale, quats, viewmat12, fx, fy, cx, cy, img_h, img_w,
                                     block_width, clip_thresh, cov3d, xys, depths, radii, conics, compensation,
                                     num_tiles_hit, check_quats ? (rb.direct ? rb.direct : flag_dev) : nullptr, quat_tol,
                                     stamp, rb.direct ? rb.direct + 1 : nullptr, semantics, stream);
    if (rc) return rc;
    if (check_quats) {
        if (!rb.direct) {                   // the copy command is the transport: its completion is the landing
            rb.src = n > 0 ? flag_dev : nullptr;
            if (n < 1) rb.host[0] = 0;
            rb.host[1] = stamp;
        }
        if (!rb.polled && flag_pinned) flag_pinned[2] = -stamp;
        if ((rc = rb.queue(s))) return rc;
    }
    if (gid_by_rank != nullptr && n > 0) {
        rc = sgn_depth_rank(n, depths, radii, gid_by_rank, rank_ws, rank_ws_bytes, sort_rank_mode, stream);
        if (rc) return rc;
    }
    if (check_quats == 1) {
        // the ranking is queued behind the projection: wait now
        const hipError_t e = rb.wait(s);
        if (e != hipSuccess) return hip_fail("sgn_project_fwd_all", e);
        int32_t bad = 0;
        rc = read_quat_flag(rb.host, stamp, &bad, "sgn_project_fwd_all");
        if (rc) return rc;
        *quats_bad_host = (n > 0 && bad) ? 1 : 0;
    }
    return 0;
}

// The wait of a sgn_project_fwd_all(check_quats = 2) call, made by the same thread on the same device: the caller does
// its own host-side bookkeeping for the projection's outputs first, while the flag is still on its way (the device is
// busy behind it; what the host does before this wait is off the critical path).  The check has its own event, so other
// calls of this library may come in between.
SGN_EXPORT
int sgn_project_check_wait(const int32_t *flag_pinned, int32_t flag_stamp, int32_t *quats_bad_host,
                           sgn_stream_t stream) {
    if (!flag_pinned || !quats_bad_host) { sgn_set_error("sgn_project_check_wait: NULL argument"); return -1; }
    const int32_t stamp = flag_stamp > 0 ? flag_stamp : 1;
    ReadBack rb = quats_readback("sgn_project_check_wait", stamp);
    rb.host = const_cast<int32_t *>(flag_pinned);
    rb.polled = ((const volatile int32_t *)flag_pinned)[2] != -stamp;     // -stamp: the call went the copy + event way
    if (!rb.polled && cached_event(EV_QUATS_CHECK, &rb.ev) != 0) { sgn_set_error("sgn_project_check_wait: no event"); return -2; }
    const hipError_t e = rb.wait((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail("sgn_project_check_wait", e);
    return read_quat_flag(flag_pinned, stamp, quats_bad_host, "sgn_project_check_wait");
}

// ---------------------------------------------------------------- the forward of a rasterize node, one call
// forward_all: the sequence shared by sgn_rasterize_fwd_all (one image) and sgn_rasterize_views_fwd_all (all rows of
// n_views views at once: ONE depth ranking, ONE host wait, ONE emission / tile sort / launch order over the n_views *
// tiles tiles — tile id = view * tiles + local tile — and ONE launch of the forward kernels): first half of the
// binning, the asynchronous read-back of the intersection count, the per-Gaussian rows, the SPECULATIVE second half of
// the binning (emission + tile sort + bins sized by the caller's capacity, the true count read on the device), the wait
// for the count — the path's one host sync —, the capacity check, the launch order and the forward kernels.
namespace {
struct ForwardPlan {
    const char *fn;
    int n_views;                     // 0: one image (sgn_bin_intersect_zero, sgn_raster_fwd[_precleared]); >= 1: batched
                                     // (sgn_bin_intersect_views, sgn_raster_views_fwd, which does not clear tile_stats itself)
    const float *opacity_logits;     // batched: the per-Gaussian logits, repeated per view into the arena (the rows' opacities)
    bool may_poll;                   // the count may go straight from the scan into a mapped count_pinned, `extra` with it,
                                     // and be polled (batched: always copy + event, one wait per batch either way)
};

int forward_all(const ForwardPlan &plan, int n, const float *xys, const float *depths, const int32_t *radii,
                const float *conics, const float *colors, const float *opacities, int opacity_is_logit, int cull,
                int img_h, int img_w, int block_width, const float *background3, const int32_t *gid_by_rank_ready,
                int quadrant_masks, float *out_img, float *final_Ts, int32_t *final_idx, float *out_depth,
                int32_t *gaussian_ids_sorted, int64_t isect_capacity, int32_t *tile_bins, int32_t *tile_order,
                int32_t *tile_stats, void *rows, size_t rows_bytes, void *order_scratch, size_t order_scratch_bytes,
                void *arena, int32_t *count_pinned, const int32_t *extra_dev, int32_t *extra_pinned,
                int64_t *n_isect_host, int sort_rank_mode, int semantics, const sgn_raster_opts *opts,
                sgn_stream_t stream) {
    const bool batched = plan.n_views > 0;
    hipStream_t s = (hipStream_t)stream;
    const TileGrid g = tile_grid(img_h, img_w, block_width);       // (one view's grid: every view shares it)
    const int n_tiles = g.n * (batched ? plan.n_views : 1);
    const ForwardArena a(arena, n, isect_capacity, batched);
    int32_t *gid = gid_by_rank_ready ? const_cast<int32_t *>(gid_by_rank_ready) : a.gid;
    int rc = 0;
    if (batched) {
        if ((rc = sgn_views_repeat(n / plan.n_views, plan.n_views, plan.opacity_logits, a.repeat, stream))) return rc;
        opacities = a.repeat;
    }
    const int do_cull = (cull && conics && opacities) ? 1 : 0;
    // everything queued between rb.queue and rb.wait runs while the count travels
    ReadBack rb(plan.fn, "count", EV_COUNT_WAIT, 0, -1, -1, -1);
    int32_t pageable = -1;
    int32_t *count_dev = a.cum_r + (n - 1);
    rb.src = count_dev; rb.extra_src = extra_dev; rb.extra_host = extra_pinned;
    rb.arm(count_pinned, &pageable, plan.may_poll ? ReadBack::ALWAYS : ReadBack::NEVER);
    rc = sgn_bin_prepare_total(n, xys, depths, radii, do_cull ? conics : nullptr, do_cull ? opacities : nullptr,
                               opacity_is_logit, do_cull, g.x, g.y, block_width, a.cum_r, gid, gid_by_rank_ready ? 1 : 0,
                               a.bin_recs, a.ws1, a.ws1_bytes, sort_rank_mode, rb.direct,
                               rb.extra_direct ? extra_dev : nullptr, rb.extra_direct, semantics, stream);
    if (rc) return rc;
    if ((rc = rb.queue(s))) return rc;
    rc = sgn_raster_build_rows(n, xys, conics, colors, opacities, opacity_is_logit, 0, n, 0, rows, rows_bytes, nullptr, stream);
    if (rc) return rc;
    // tile_stats laid out right behind tile_bins (ONE buffer of the caller's): the emission clears both, and neither the
    // bins nor the statistics cost a clear launch of their own
    const bool stats_behind_bins = tile_stats == tile_bins + 2 * (size_t)n_tiles;
    const int also_zero = stats_behind_bins ? 2 * n_tiles : 0;
    rc = batched ? sgn_bin_intersect_views(plan.n_views, n, isect_capacity, a.bin_recs, a.cum_r, gid, g.x, g.y,
                                           gaussian_ids_sorted, tile_bins, quadrant_masks, a.ws2, a.ws2_bytes, count_dev,
                                           sort_rank_mode, also_zero, stream)
                 : sgn_bin_intersect_zero(n, isect_capacity, a.bin_recs, a.cum_r, gid, g.x, g.y, block_width,
                                          gaussian_ids_sorted, tile_bins, quadrant_masks, a.ws2, a.ws2_bytes, count_dev,
                                          sort_rank_mode, also_zero, stream);
    if (rc) return rc;
    hipError_t e = rb.wait(s);
    if (e != hipSuccess) { sgn_set_error("%s%s: %s", plan.fn, rb.cold ? ": count copy" : "", hipGetErrorString(e)); return (int)e; }
    const int64_t count = (int64_t)*(volatile int32_t *)rb.host;
    *n_isect_host = count;
    if (count > isect_capacity) return SGN_E_CAPACITY;   // the list did not fit: call again with more room
    if (count < 1) return 0;                             // nothing visible: the caller writes the background image
    if (batched && !stats_behind_bins) {
        e = hipMemsetAsync(tile_stats, 0, sizeof(int32_t) * 2 * (size_t)n_tiles, s);
        if (e != hipSuccess) return hip_fail(plan.fn, e);
    }
    const sgn_raster_opts o = opts_or_default(opts);
    rc = sgn_tile_order(n_tiles, tile_bins, nullptr, fwd_long_thresh(o, block_width), 0, tile_order, order_scratch,
                        order_scratch_bytes, stream);
    if (rc) return rc;
    sgn_raster_opts oo = o;
    oo.ids_qmask = quadrant_masks ? 1 : 0;
    // out_depth: the DEPTH CHANNEL rides the colour pass (sgn_raster_fwd's depths / out_depth; the scene graph's and the
    // reference's depth pass is then answered from it, sgn_depth_reuse)
    const float *dch = out_depth ? depths : nullptr;
    if (batched)
        return sgn_raster_views_fwd(plan.n_views, img_h, img_w, gaussian_ids_sorted, tile_bins, rows, background3, out_img,
                                    final_Ts, final_idx, tile_order, tile_stats, dch, out_depth, &oo, stream);
    if (stats_behind_bins)
        return sgn_raster_fwd_precleared(img_h, img_w, block_width, n, count, gaussian_ids_sorted, tile_bins, xys, conics,
                                         colors, opacities, opacity_is_logit, background3, out_img, final_Ts, final_idx,
                                         rows, rows_bytes, tile_order, tile_stats, dch, out_depth, &oo, stream);
    return sgn_raster_fwd(img_h, img_w, block_width, n, count, gaussian_ids_sorted, tile_bins, xys, conics, colors,
                          opacities, opacity_is_logit, 0, n, 0, background3, out_img, final_Ts, final_idx, rows,
                          rows_bytes, 1, tile_order, tile_stats, dch, out_depth, nullptr, &oo, stream);
}
}  // namespace

SGN_EXPORT size_t sgn_rasterize_arena_bytes(int n, int64_t isect_capacity) {
    return ForwardArena(nullptr, n, isect_capacity, false).bytes;
}

// sgn_rasterize_fwd_all: the whole forward of `rasterize_gaussians` for the plain case (the full scene, gather mode).
SGN_EXPORT
int sgn_rasterize_fwd_all(int n, const float *xys, const float *depths, const int32_t *radii, const float *conics,
                          const float *colors, const float *opacities, int opacity_is_logit, int cull, int img_h,
                          int img_w, int block_width, const float *background3, const int32_t *gid_by_rank_ready,
                          int quadrant_masks, float *out_img, float *final_Ts, int32_t *final_idx, float *out_depth,
                          int32_t *gaussian_ids_sorted, int64_t isect_capacity, int32_t *tile_bins,
                          int32_t *tile_order, int32_t *tile_stats, void *rows, size_t rows_bytes,
                          void *order_scratch, size_t order_scratch_bytes, void *arena, size_t arena_bytes,
                          int32_t *count_pinned, const int32_t *extra_dev, int32_t *extra_pinned,
                          int64_t *n_isect_host, int sort_rank_mode, int semantics, const sgn_raster_opts *opts,
                          sgn_stream_t stream) {
    if (n < 1 || !xys || !depths || !radii || !colors || !opacities || !background3 || !out_img || !final_Ts ||
        !final_idx || !gaussian_ids_sorted || !tile_bins || !tile_order || !tile_stats || !rows || !arena ||
        !n_isect_host || isect_capacity < 1 || block_width < 2 || block_width > 16 || img_h < 1 || img_w < 1) {
        sgn_set_error("sgn_rasterize_fwd_all: argument check failed");
        return -1;
    }
    if (arena_bytes < sgn_rasterize_arena_bytes(n, isect_capacity)) {
        sgn_set_error("sgn_rasterize_fwd_all: arena too small");
        return -2;
    }
    const ForwardPlan plan{"sgn_rasterize_fwd_all", 0, nullptr, true};
    return forward_all(plan, n, xys, depths, radii, conics, colors, opacities, opacity_is_logit, cull, img_h, img_w,
                       block_width, background3, gid_by_rank_ready, quadrant_masks, out_img, final_Ts, final_idx,
                       out_depth, gaussian_ids_sorted, isect_capacity, tile_bins, tile_order, tile_stats, rows, rows_bytes,
                       order_scratch, order_scratch_bytes, arena, count_pinned, extra_dev, extra_pinned, n_isect_host,
                       sort_rank_mode, semantics, opts, stream);
}

// ---------------------------------------------------------------- a sub-model pass over a CACHED list, one call (round 6)
// sgn_rasterize_window_all: the forward of a `rasterize_gaussians` call whose tensors are a ROW WINDOW of a scene that was
// binned a moment ago (the scene graph's objects-only / background-only accumulation passes,
// sgn_splatfacto_scene_graph.py:364-366: torch.cat copies of per-model slices of the main projection): the device-side
// comparison that proves it (sgn_rows_match over whichever tensor pairs are given, at up to 4 candidate offsets), the
// read-back of its verdict — this path's one host sync, in place of the intersection count's read-back of the binning it
// saves —, the window's rows, its own compacted sub-list (sgn_list_window) when asked for, the launch order and the
// forward kernels, on `stream`, temporaries from one arena.  *matched_lo_host = the matching offset, or -1: nothing matched,
// nothing was rasterized, the caller bins the tensors as a scene of their own.
SGN_EXPORT size_t sgn_rasterize_window_arena_bytes(int n_tiles) { return WindowArena(nullptr, n_tiles).bytes; }

SGN_EXPORT
int sgn_rasterize_window_all(int n_win, int n_full, int n_cand, const int32_t *cand_lo_host, const float *xys_w,
                             const float *depths_w, const int32_t *radii_w, const int32_t *num_tiles_hit_w,
                             const float *conics_w, const float *colors_w, const float *opacities_w,
                             int opacity_is_logit, const float *xys, const float *depths, const int32_t *radii,
                             const int32_t *num_tiles_hit, const float *conics, const float *opacities,
                             int64_t n_isect, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                             int ids_qmask, int img_h, int img_w, int block_width, const float *background3,
                             int sub_list, const int32_t *tile_order_ready, float *out_img, float *final_Ts,
                             int32_t *final_idx, int32_t *ids_out, int32_t *tile_bins_out, int32_t *tile_order,
                             int32_t *tile_stats, void *rows, size_t rows_bytes, void *order_scratch,
                             size_t order_scratch_bytes, void *arena, size_t arena_bytes, int32_t *verdict_pinned,
                             int *matched_lo_host, const sgn_raster_opts *opts, sgn_stream_t stream) {
    if (n_win < 1 || n_full < n_win || n_cand < 1 || n_cand > 4 || !cand_lo_host || !xys_w || !conics_w || !colors_w ||
        !opacities_w || !gaussian_ids_sorted || !tile_bins || !background3 || !out_img || !final_Ts || !final_idx ||
        !tile_stats || !rows || !arena || !matched_lo_host || n_isect < 1 || block_width < 2 || block_width > 16 ||
        img_h < 1 || img_w < 1 || (sub_list && (!ids_out || !tile_bins_out)) || (!tile_order_ready && !tile_order)) {
        sgn_set_error("sgn_rasterize_window_all: argument check failed");
        return -1;
    }
    const int n_tiles = tile_grid(img_h, img_w, block_width).n;
    if (arena_bytes < sgn_rasterize_window_arena_bytes(n_tiles)) {
        sgn_set_error("sgn_rasterize_window_all: arena too small");
        return -2;
    }
    const sgn_raster_opts o = opts_or_default(opts);
    hipStream_t s = (hipStream_t)stream;
    const WindowArena a(arena, n_tiles);
    *matched_lo_host = -1;
    int lo = -1;
    const bool compare = xys || depths || radii || num_tiles_hit || conics || opacities;
    if (compare) {
        int rc = sgn_rows_match(n_win, n_full, n_cand, cand_lo_host, xys ? xys_w : nullptr, depths ? depths_w : nullptr,
                                radii ? radii_w : nullptr, num_tiles_hit ? num_tiles_hit_w : nullptr,
                                conics ? conics_w : nullptr, opacities ? opacities_w : nullptr, xys, depths, radii,
                                num_tiles_hit, conics, opacities, a.mismatch, stream);
        if (rc) return rc;
        // verdict_pinned is EIGHT words: [0, 4) the verdicts, [7] "they have landed" (polled)
        int32_t pageable[8] = {1, 1, 1, 1, 0, 0, 0, 0};
        ReadBack rb("sgn_rasterize_window_all", "verdict", EV_COUNT_WAIT, 7, 0, 1, n_cand);
        rb.src = a.mismatch; rb.n_words = n_cand;
        rb.arm(verdict_pinned, pageable, ReadBack::IF_POLLED);
        if ((rc = rb.queue(s))) return rc;
        const hipError_t e = rb.wait(s);
        if (e != hipSuccess) return hip_fail("sgn_rasterize_window_all: verdict read-back", e);
        for (int c = 0; c < n_cand && lo < 0; ++c)
            if (((volatile int32_t *)rb.host)[c] == 0) lo = cand_lo_host[c];
        if (lo < 0) return 0;                   // not a window of that scene: the caller re-bins
    } else {
        lo = cand_lo_host[0];                   // the caller has settled every tensor another way
        if (lo < 0 || lo + n_win > n_full) { sgn_set_error("sgn_rasterize_window_all: offset out of range"); return -4; }
    }
    *matched_lo_host = lo;
    const int id_lo = lo, id_hi = lo + n_win;
    int rc = sgn_raster_build_rows(n_full, xys_w, conics_w, colors_w, opacities_w, opacity_is_logit, id_lo, id_hi, 1,
                                   rows, rows_bytes, nullptr, stream);
    if (rc) return rc;
    const int32_t *ids = gaussian_ids_sorted, *bins = tile_bins;
    const int32_t *order = tile_order_ready;
    if (sub_list) {      // a SMALL window walks its own entries only (same relative order: same image and gradients)
        rc = sgn_list_window(n_tiles, gaussian_ids_sorted, tile_bins, id_lo, id_hi, ids_qmask, ids_out, tile_bins_out,
                             a.lw_ws, a.lw_bytes, stream);
        if (rc) return rc;
        ids = ids_out; bins = tile_bins_out;
        order = nullptr;                        // another list: another order
    }
    if (!order) {
        rc = sgn_tile_order(n_tiles, bins, nullptr, fwd_long_thresh(o, block_width), 0, tile_order, order_scratch,
                            order_scratch_bytes, stream);
        if (rc) return rc;
        order = tile_order;
    }
    sgn_raster_opts oo = o;
    oo.ids_qmask = ids_qmask ? 1 : 0;
    return sgn_raster_fwd(img_h, img_w, block_width, n_full, n_isect, ids, bins, xys_w, conics_w, colors_w, opacities_w,
                          opacity_is_logit, id_lo, id_hi, 1, background3, out_img, final_Ts, final_idx, rows, rows_bytes,
                          1, order, tile_stats, nullptr, nullptr, nullptr, &oo, stream);
}

// ---------------------------------------------------------------- the backward of a rasterize node, one call (round 6)
// sgn_rasterize_bwd_all = sgn_tile_order (the reverse walks' launch order, from the forward's tile statistics) +
// sgn_raster_bwd / sgn_raster_bwd_part.  tile_order [tiles + 2] stays the caller's (its last word is the walked / listed
// statistic the host's quadrant-mask policy reads back later).  first / last as in sgn_raster_bwd_part; first = last = 1 is
// the plain sgn_raster_bwd (window allowed).
SGN_EXPORT
int sgn_rasterize_bwd_all(int img_h, int img_w, int block_width, int n, int64_t n_isect,
                          const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const int32_t *tile_stats,
                          int stats_have_pairs, const float *xys, const float *conics, const float *colors,
                          const float *opacities, int opacity_is_logit, int id_lo, int id_hi, int window,
                          const float *background3, const float *final_Ts, const int32_t *final_idx,
                          const float *v_out_img, const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy,
                          float *v_conic, float *v_colors, float *v_opacity, void *recs_ws, size_t recs_ws_bytes,
                          int recs_packed, void *grad_ws, size_t grad_ws_bytes, int32_t *tile_order,
                          void *order_scratch, size_t order_scratch_bytes, int small_q16,
                          const float *colors_pre_clamp, const sgn_raster_opts *opts, sgn_stream_t stream,
                          sgn_stream_t aux_stream, int first, int last) {
    const sgn_raster_opts o = opts_or_default(opts);
    const int32_t *order = nullptr;
    if (tile_order != nullptr && n_isect > 0 && n > 0) {
        if (!tile_bins || !tile_stats) { sgn_set_error("sgn_rasterize_bwd_all: tile_order needs tile_bins and tile_stats"); return -1; }
        int rc = sgn_tile_order(tile_grid(img_h, img_w, block_width).n, tile_bins, tile_stats, o.adapt_bwd > 0 ? o.adapt_bwd : 256,
                                stats_have_pairs ? small_q16 : 0, tile_order, order_scratch, order_scratch_bytes, stream);
        if (rc) return rc;
        order = tile_order;
    }
    if (first && last)
        return sgn_raster_bwd(img_h, img_w, block_width, n, n_isect, gaussian_ids_sorted, tile_bins, xys, conics, colors,
                              opacities, opacity_is_logit, id_lo, id_hi, window, background3, final_Ts, final_idx,
                              v_out_img, v_out_alpha, alpha_clamp_bwd, v_xy, v_conic, v_colors, v_opacity, recs_ws,
                              recs_ws_bytes, recs_packed, grad_ws, grad_ws_bytes, order, colors_pre_clamp, opts, stream,
                              aux_stream);
    return sgn_raster_bwd_part(img_h, img_w, block_width, n, n_isect, gaussian_ids_sorted, tile_bins, xys, conics, colors,
                               opacities, opacity_is_logit, id_lo, id_hi, window, background3, final_Ts, final_idx,
                               v_out_img, v_out_alpha, alpha_clamp_bwd, v_xy, v_conic, v_colors, v_opacity, recs_ws,
                               recs_ws_bytes, recs_packed, grad_ws, grad_ws_bytes, order, colors_pre_clamp, opts, stream,
                               aux_stream, first, last);
}

// ---------------------------------------------------------------- batched views, one call per direction
// sgn_rasterize_views_fwd_all: forward_all over the rows of all n_views views at once.
SGN_EXPORT size_t sgn_rasterize_views_arena_bytes(int n_views, int n, int64_t isect_capacity) {
    if (n_views < 1 || n_views > SGN_VIEWS_MAX || n < 0) return 0;
    return ForwardArena(nullptr, n_views * n, isect_capacity, true).bytes;
}

SGN_EXPORT
int sgn_rasterize_views_fwd_all(int n_views, int n, const float *xys, const float *depths, const int32_t *radii,
                                const float *conics, const float *colors, const float *opacity_logits, int cull,
                                int img_h, int img_w, int block_width, const float *background3, int quadrant_masks,
                                float *out_img, float *final_Ts, int32_t *final_idx, float *out_depth,
                                int32_t *gaussian_ids_sorted, int64_t isect_capacity, int32_t *tile_bins,
                                int32_t *tile_order, int32_t *tile_stats, void *rows, size_t rows_bytes,
                                void *order_scratch, size_t order_scratch_bytes, void *arena, size_t arena_bytes,
                                int32_t *count_pinned, int64_t *n_isect_host, int sort_rank_mode, int semantics,
                                const sgn_raster_opts *opts, sgn_stream_t stream) {
    if (int rc = views_args(__func__, n_views, n)) return rc;
    if (block_width != 16 || img_h < 1 || img_w < 1) {
        sgn_set_error("sgn_rasterize_views_fwd_all: needs block_width 16 and a positive image size");
        return -3;
    }
    if (!n_isect_host || (n > 0 && (!xys || !depths || !radii || !conics || !colors || !opacity_logits ||
                                    !background3 || !out_img || !final_Ts || !final_idx || !gaussian_ids_sorted ||
                                    !tile_bins || !tile_order || !tile_stats || !rows || !arena))) {
        sgn_set_error("sgn_rasterize_views_fwd_all: a required pointer is NULL");
        return -4;
    }
    *n_isect_host = 0;
    if (n == 0) return 0;
    if (isect_capacity < 1 || isect_capacity >= ((int64_t)1 << 31)) {
        sgn_set_error("sgn_rasterize_views_fwd_all: isect_capacity %lld", (long long)isect_capacity);
        return -6;
    }
    const int R = n_views * n;
    if (arena_bytes < sgn_rasterize_views_arena_bytes(n_views, n, isect_capacity) ||
        rows_bytes < sgn_raster_workspace_bytes(R, 0, nullptr)) {
        sgn_set_error("sgn_rasterize_views_fwd_all: arena or rows too small");
        return -5;
    }
    const ForwardPlan plan{"sgn_rasterize_views_fwd_all", n_views, opacity_logits, false};
    return forward_all(plan, R, xys, depths, radii, conics, colors, nullptr, 1, cull, img_h, img_w, 16, background3,
                       nullptr, quadrant_masks, out_img, final_Ts, final_idx, out_depth, gaussian_ids_sorted,
                       isect_capacity, tile_bins, tile_order, tile_stats, rows, rows_bytes, order_scratch,
                       order_scratch_bytes, arena, count_pinned, nullptr, nullptr, n_isect_host, sort_rank_mode, semantics,
                       opts, stream);
}

SGN_EXPORT
int sgn_rasterize_views_bwd_all(int n_views, int n, int64_t n_isect, int img_h, int img_w,
                                const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, const int32_t *tile_stats,
                                const float *conics, const float *opacity_logits, const float *background3,
                                const float *final_Ts, const int32_t *final_idx, const float *v_out_img,
                                const float *v_out_alpha, float alpha_clamp_bwd, float *v_xy, float *v_conic,
                                float *v_colors, float *v_opacity_logits, const void *rows, size_t rows_bytes,
                                void *grad_ws, size_t grad_ws_bytes, int32_t *tile_order, void *order_scratch,
                                size_t order_scratch_bytes, int small_q16, const sgn_raster_opts *opts,
                                sgn_stream_t stream, sgn_stream_t aux_stream) {
    if (int rc = views_args(__func__, n_views, n)) return rc;
    if (img_h < 1 || img_w < 1 || !(alpha_clamp_bwd > 0.f && alpha_clamp_bwd < 1.f)) {
        sgn_set_error("sgn_rasterize_views_bwd_all: bad image size or alpha clamp");
        return -3;
    }
    if (n == 0) return 0;
    if (!conics || !opacity_logits || !v_xy || !v_conic || !v_colors || !v_opacity_logits || !grad_ws || !rows ||
        (n_isect > 0 && (!gaussian_ids_sorted || !tile_bins || !tile_stats || !tile_order || !background3 ||
                         !final_Ts || !final_idx || !v_out_alpha))) {
        sgn_set_error("sgn_rasterize_views_bwd_all: a required pointer is NULL");
        return -4;
    }
    const int R = n_views * n;
    if (grad_ws_bytes < sgn_raster_bwd_workspace_bytes(R) || rows_bytes < sgn_raster_workspace_bytes(R, 0, nullptr)) {
        sgn_set_error("sgn_rasterize_views_bwd_all: workspace too small");
        return -5;
    }
    if (n_isect < 0 || n_isect >= ((int64_t)1 << 31)) {
        sgn_set_error("sgn_rasterize_views_bwd_all: n_isect %lld", (long long)n_isect);
        return -6;
    }
    const sgn_raster_opts o = opts_or_default(opts);
    const int n_tiles = tile_grid(img_h, img_w, 16).n * n_views;
    if (n_isect > 0) {
        int rc = sgn_tile_order(n_tiles, tile_bins, tile_stats, o.adapt_bwd > 0 ? o.adapt_bwd : 256, small_q16,
                                tile_order, order_scratch, order_scratch_bytes, stream);
        if (rc) return rc;
    } else {
        // nothing was listed: every gradient is zero (the walks find empty lists; the unpack writes zeros)
        const hipError_t e = hipMemsetAsync(tile_order, 0, sizeof(int32_t) * ((size_t)n_tiles + 2), (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail("sgn_rasterize_views_bwd_all", e);
    }
    return sgn_raster_views_bwd(n_views, n, img_h, img_w, gaussian_ids_sorted, tile_bins, rows, conics,
                                opacity_logits, background3, final_Ts, final_idx, v_out_img, v_out_alpha,
                                alpha_clamp_bwd, v_xy, v_conic, v_colors, v_opacity_logits, grad_ws, tile_order, opts,
                                stream, aux_stream);
}

// ---------------------------------------------------------------- the ground-truth pyramid (gt_pyramid.hip)
SGN_EXPORT
int sgn_gt_downscale(int h, int w, int oh, int ow, const unsigned char *image, const unsigned char *mask,
                     const unsigned char *semantic, float *image_out, unsigned char *mask_out,
                     unsigned char *semantic_out, sgn_stream_t stream) {
    constexpr int MAX_DIM = 16384;                     // 32-bit element indices: 16384 * 16384 * 3 < 2^31
    SGN_ARG_CHECK(h >= 1 && w >= 1 && oh >= 1 && ow >= 1 && h <= MAX_DIM && w <= MAX_DIM, -1);
    SGN_ARG_CHECK(oh <= h && ow <= w, -1);
    SGN_ARG_CHECK(image && image_out, -2);
    SGN_ARG_CHECK((mask != nullptr) == (mask_out != nullptr), -2);
    SGN_ARG_CHECK((semantic != nullptr) == (semantic_out != nullptr), -2);
    return sgn_gt_downscale_launch(h, w, oh, ow, image, mask, semantic, image_out, mask_out, semantic_out, stream);
}

// ---------------------------------------------------------------- eval outputs as writer bytes (frame_pack.hip)
SGN_EXPORT
int sgn_frames_pack(int h, int w, int n_panels, const sgn_panel *panels, uint8_t *canvas, int canvas_h, int canvas_w,
                    sgn_stream_t stream) {
    constexpr int MAX_DIM = 16384;                     // 32-bit element indices: 16384 * 16384 * 3 < 2^31
    SGN_ARG_CHECK(h >= 1 && w >= 1 && canvas_h >= 1 && canvas_w >= 1, -1);
    SGN_ARG_CHECK(h <= MAX_DIM && w <= MAX_DIM && canvas_h <= MAX_DIM && canvas_w <= MAX_DIM, -1);
    SGN_ARG_CHECK(n_panels >= 1 && n_panels <= SGN_FRAMES_MAX_PANELS, -1);
    SGN_ARG_CHECK(panels && canvas, -2);
    for (int i = 0; i < n_panels; ++i) {
        const sgn_panel &p = panels[i];
        SGN_ARG_CHECK(p.kind == SGN_PANEL_RGB || p.kind == SGN_PANEL_SCALAR || p.kind == SGN_PANEL_BYTES, -1);
        SGN_ARG_CHECK(p.y0 >= 0 && p.x0 >= 0 && p.y0 <= canvas_h - h && p.x0 <= canvas_w - w, -1);
        SGN_ARG_CHECK(p.kind != SGN_PANEL_SCALAR || (std::isfinite(p.den) && p.den != 0.0f), -1);
        for (int j = 0; j < i; ++j) {
            const sgn_panel &o = panels[j];
            const bool panels_do_not_overlap = p.y0 >= o.y0 + h || o.y0 >= p.y0 + h || p.x0 >= o.x0 + w || o.x0 >= p.x0 + w;
            SGN_ARG_CHECK(panels_do_not_overlap, -1);
        }
    }
    for (int i = 0; i < n_panels; ++i) {
        SGN_ARG_CHECK(panels[i].src, -2);
        SGN_ARG_CHECK(panels[i].kind != SGN_PANEL_SCALAR || panels[i].lut, -2);
    }
    return sgn_frames_pack_launch(h, w, n_panels, panels, canvas, canvas_w, stream);
}

// ---------------------------------------------------------------- bilateral-grid colour correction (bilagrid.hip)
namespace {
// the checks the two entries share; 1: nothing to do
int bilagrid_check(const char *fn, int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb) {
    constexpr int MAX_DIM = 16384;                     // 32-bit element indices: 16384 * 16384 * 3 < 2^31
    SGN_ARG_CHECK_FN(fn, L >= 1 && Hg >= 1 && Wg >= 1 && H >= 1 && W >= 1, -1);
    SGN_ARG_CHECK_FN(fn, H <= MAX_DIM && W <= MAX_DIM, -1);
    SGN_ARG_CHECK_FN(fn, (int64_t)L * Hg * Wg <= ((int64_t)1 << 27), -1);          // 12 floats per cell, 32-bit offsets
    SGN_ARG_CHECK_FN(fn, n_pix >= 0 && (int64_t)n_pix <= (int64_t)H * W, -1);
    if (n_pix == 0) return 1;
    SGN_ARG_CHECK_FN(fn, grid && rgb, -2);
    SGN_ARG_CHECK_FN(fn, ((uintptr_t)grid & 15) == 0, -3);                         // cells are read 16 bytes at a time
    return 0;
}
}  // namespace

SGN_EXPORT
int sgn_bilagrid_slice_fwd(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                           float *out, sgn_stream_t stream) {
    if (int rc = bilagrid_check(__func__, L, Hg, Wg, grid, H, W, n_pix, rgb)) return rc < 0 ? rc : 0;
    SGN_ARG_CHECK(out, -2);
    return sgn_bilagrid_slice_fwd_launch(L, Hg, Wg, grid, H, W, n_pix, rgb, out, stream);
}

SGN_EXPORT
int sgn_bilagrid_slice_bwd(int L, int Hg, int Wg, const float *grid, int H, int W, int n_pix, const float *rgb,
                           const float *v_out, float *v_rgb, float *v_grid, sgn_stream_t stream) {
    if (int rc = bilagrid_check(__func__, L, Hg, Wg, grid, H, W, n_pix, rgb)) return rc < 0 ? rc : 0;
    SGN_ARG_CHECK(v_out, -2);
    if (v_rgb == nullptr && v_grid == nullptr) return 0;                           // neither gradient is wanted
    return sgn_bilagrid_slice_bwd_launch(L, Hg, Wg, grid, H, W, n_pix, rgb, v_out, v_rgb, v_grid, stream);
}

// ---------------------------------------------------------------- kernel timing (bench/profiles)
// Opt-in: when enabled every timed launch is bracketed by hipEventRecord on the SAME stream the
// kernel is launched on; sgn_timing_get() synchronises the recorded events and sums them.
namespace {
struct Span { hipEvent_t a, b; int slot; };
std::mutex g_mu;
std::vector<Span> g_spans;
int g_timing = 0;
}  // namespace

int sgn_timing_enabled() { return g_timing; }

void sgn_timing_begin(int slot, void *stream) {
    if (!g_timing) return;
    Span s;
    s.slot = slot;
    if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
    (void)hipEventRecord(s.a, (hipStream_t)stream);
    std::lock_guard<std::mutex> lk(g_mu);
    g_spans.push_back(s);
}

void sgn_timing_end(int slot, void *stream) {
    if (!g_timing) return;
    std::lock_guard<std::mutex> lk(g_mu);
    for (size_t i = g_spans.size(); i-- > 0;)
        if (g_spans[i].slot == slot) { (void)hipEventRecord(g_spans[i].b, (hipStream_t)stream); return; }
}

// host microseconds the calling thread has spent blocked in the event waits of the one-call entries (sgn_project_fwd_all /
// sgn_project_check_wait, sgn_rasterize_fwd_all, sgn_rasterize_window_all) since the last reset, and how many waits
SGN_EXPORT double sgn_timing_host_wait_us(int reset, int64_t *n_waits) {
    const double t = g_wait_us;
    if (n_waits) *n_waits = g_wait_n;
    if (reset) { g_wait_us = 0.0; g_wait_n = 0; }
    return t;
}

SGN_EXPORT void sgn_timing_enable(int on) {
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto &s : g_spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    g_spans.clear();
    g_timing = on ? 1 : 0;
}

SGN_EXPORT int sgn_timing_get(int slot, int *count, float *total_ms) {
    std::lock_guard<std::mutex> lk(g_mu);
    int c = 0;
    float t = 0.f;
    for (auto &s : g_spans) {
        if (s.slot != slot) continue;
        if (hipEventSynchronize(s.b) != hipSuccess) return 1;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) return 2;
        t += ms;
        ++c;
    }
    if (count) *count = c;
    if (total_ms) *total_ms = t;
    return 0;
}
