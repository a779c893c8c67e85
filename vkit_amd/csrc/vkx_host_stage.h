// Host-plane staging of the host-pointer entry points (vkx_X next to vkx_X_dev): HostStage moves the caller's planes to the
// device and back; vkx_host_run states one entry point as its planes plus the call of its _dev form.  Shared by host_api.hip
// and by the kernel files that keep a host form next to its _dev form.
#pragma once
#include "vkx_internal.h"

#include <initializer_list>
#include <stdlib.h>
#include <string.h>

// Collects the planes of one call, packs them into a single device allocation (stage[0]) and moves them with
// hipMemcpy2DAsync so arbitrary host row pitches are honoured.  commit(), commit_mapped() and finish() bind the context's
// device themselves (vkx_device_guard: free when it is current already), so a host call is safe from any thread.
class HostStage {
public:
    explicit HostStage(vkx_ctx *ctx) : ctx_(ctx), mapped_(ctx) {}

    // returns the plane id; device pitch is row_bytes (tightly packed)
    int add(const void *host_in, void *host_out, size_t row_bytes, int rows, ptrdiff_t host_pitch)
    {
        Plane p;
        p.in = host_in; p.out = host_out; p.row_bytes = row_bytes; p.rows = rows; p.pitch = host_pitch;
        p.off = total_;
        if (rows > 1 && (host_pitch < 0 || (size_t)host_pitch < row_bytes)) bad_pitch_ = true;   // vkx.h: a pitch of at least one row
        total_ += vkx_align256(row_bytes * (size_t)(rows > 0 ? rows : 0));
        planes_.push_back(p);
        return (int)planes_.size() - 1;
    }

    // copy_aside: the call is asynchronous (nothing is read back): its staging copy may go to the copy stream (see below)
    int commit(bool copy_aside = false)
    {
        if (bad_pitch_) {
            vkx_set_error("host plane with a row pitch shorter than its row, or negative");
            return VKX_ERR_INVALID;
        }
        vkx_device_guard guard(ctx_);
        int rc = vkx_scratch_reserve(ctx_, &ctx_->stage[0], total_ ? total_ : 256);
        if (rc) return rc;
        base_ = (uint8_t *)ctx_->stage[0].ptr;
        // The input planes are gathered in the page-locked descriptor ring and travel as ONE copy per run of neighbours (normally one
        // run): a copy from pageable memory is staged by the runtime anyway -- in chunks, each a copy KERNEL on the compute queue (a C4
        // page's two full-page score maps were 9 such dispatches) --, while one copy out of page-locked memory goes to a DMA engine and
        // leaves the compute queue to the kernels (of this process and of the other workers sharing the GPU).  Beyond 48 MB of inputs
        // the planes go directly.
        constexpr size_t kRingMax = (size_t)48 << 20;
        size_t in_total = 0;
        for (auto &p : planes_)
            if (p.in && p.row_bytes && p.rows > 0) in_total += vkx_align256(p.row_bytes * (size_t)p.rows);
        uint8_t *ring = nullptr;
        if (in_total > 0 && in_total <= kRingMax) {
            void *r = nullptr;
            if ((rc = vkx_desc_ring_take(ctx_, in_total, &r))) return rc;
            ring = (uint8_t *)r;
        }
        size_t ring_off = 0, run_dev = 0, run_ring = 0, run_bytes = 0;
        // A page's worth of planes (>= 256 KB) is copied on the context's host -> device copy stream, ordered after what the compute stream
        // has queued (the staging block may still be read) and before what it queues next.  In line on the compute stream, behind
        // kernels, the runtime executes the copy as a copy KERNEL (8 MB: 0.2 ms of the compute queue per page); on a stream of its own it
        // goes to a DMA engine: kernel time per C4 page 0.74 -> 0.52 ms, eight workers sharing the GPU 1 202 -> 1 563 pages/s
        // (profiles/r6h0_ / r6h1_page_dispatches.txt).
        hipStream_t copy_stream = ctx_->stream;
        // (only for calls that return without reading anything back: behind a synchronous call -- similarity_mls.distort on one 2048^2
        //  image -- the DMA engine's start-up latency is what the caller waits for: 1.5 -> 2.1 ms per call)
        if (copy_aside && ring && in_total >= ((size_t)256 << 10)) {
            int src = VKX_OK;
            hipStream_t cs = vkx_stream_by_id(ctx_, VKX_STREAM_COPY_IN, &src);
            if (src == VKX_OK && cs && vkx_stream_order(ctx_, cs, ctx_->stream) == VKX_OK) copy_stream = cs;
        }
        auto flush = [&]() -> hipError_t {
            if (!run_bytes) return hipSuccess;
            const hipError_t e = hipMemcpyAsync(base_ + run_dev, ring + run_ring, run_bytes, hipMemcpyHostToDevice, copy_stream);
            run_bytes = 0;
            return e;
        };
        for (auto &p : planes_) {
            if (!p.in || p.row_bytes == 0 || p.rows <= 0) continue;
            const size_t bytes = p.row_bytes * (size_t)p.rows, padded = vkx_align256(bytes);
            if (ring) {
                // device offsets of consecutive planes are contiguous (add() pads to 256 like the ring does)
                if (run_bytes && run_dev + run_bytes != p.off) VKX_HIP(flush());
                if (!run_bytes) { run_dev = p.off; run_ring = ring_off; }
                if ((size_t)p.pitch == p.row_bytes || p.rows == 1) memcpy(ring + ring_off, p.in, bytes);
                else
                    for (int r = 0; r < p.rows; r++) memcpy(ring + ring_off + (size_t)r * p.row_bytes, (const uint8_t *)p.in + (ptrdiff_t)r * p.pitch, p.row_bytes);
                ring_off += padded;
                run_bytes += padded;
                continue;
            }
            VKX_HIP(flush());
            // a contiguous plane (the normal numpy case) is ONE linear copy: the 2-D form moves row by row and runs at a
            // fraction of the link (15 ms instead of 0.5 ms for a 2048^2 RGB page and its result)
            if ((size_t)p.pitch == p.row_bytes || p.rows == 1)
                VKX_HIP(hipMemcpyAsync(base_ + p.off, p.in, bytes, hipMemcpyHostToDevice, ctx_->stream));
            else
                VKX_HIP(hipMemcpy2DAsync(base_ + p.off, p.row_bytes, p.in, (size_t)p.pitch, p.row_bytes, (size_t)p.rows,
                                         hipMemcpyHostToDevice, ctx_->stream));
        }
        VKX_HIP(flush());
        if (copy_stream != ctx_->stream) return vkx_stream_order(ctx_, ctx_->stream, copy_stream);
        return VKX_OK;
    }

    // Input planes that the kernel reads ONCE (the layers of a composite: every pixel of a plane is touched by one lane): gathered in
    // the page-locked ring and read there, in place, over the link -- no copy to device memory at all.  The link carries each byte
    // once either way; what goes is the copy's dispatches (a C4 page staged 13 MB of layer planes with 9 runtime copy kernels) and,
    // for pageable sources, the runtime's own staging pass.  false: too large for the ring or not mappable (use commit()).
    // The ring is held (vkx_tables::mapped) until release_hold() or the end of the call: a further take of the call (the composite's
    // tile tables) cannot wrap onto the planes or free them.
    bool commit_mapped()
    {
        if (bad_pitch_ || total_ == 0 || total_ > ((size_t)48 << 20)) return false;   // commit() reports a bad pitch
        for (auto &p : planes_)
            if (p.out) return false;             // outputs need device memory + finish()
        vkx_device_guard guard(ctx_);
        if (mapped_.take(total_) != VKX_OK) return false;
        uint8_t *mapped = mapped_.mapped(), *ring = mapped_.host;
        if (!mapped) return false;
        for (auto &p : planes_) {
            if (!p.in || p.row_bytes == 0 || p.rows <= 0) continue;
            if ((size_t)p.pitch == p.row_bytes || p.rows == 1) memcpy(ring + p.off, p.in, p.row_bytes * (size_t)p.rows);
            else
                for (int row = 0; row < p.rows; row++) memcpy(ring + p.off + (size_t)row * p.row_bytes, (const uint8_t *)p.in + (ptrdiff_t)row * p.pitch, p.row_bytes);
        }
        base_ = mapped;
        return true;
    }
    // true: a take was refused while the planes were held -- the call failed for that, nothing of it is queued; commit() and run it again
    bool release_hold() { return mapped_.release(); }

    template <class T> T *dev(int id) const { return id < 0 ? nullptr : (T *)(base_ + planes_[id].off); }
    size_t total_bytes() const { return total_; }

    int finish()
    {
        vkx_device_guard guard(ctx_);
        for (auto &p : planes_) {
            if (!p.out || p.row_bytes == 0 || p.rows <= 0) continue;
            if ((size_t)p.pitch == p.row_bytes || p.rows == 1)
                VKX_HIP(hipMemcpyAsync(p.out, base_ + p.off, p.row_bytes * (size_t)p.rows, hipMemcpyDeviceToHost, ctx_->stream));
            else
                VKX_HIP(hipMemcpy2DAsync(p.out, (size_t)p.pitch, base_ + p.off, p.row_bytes, p.row_bytes, (size_t)p.rows,
                                         hipMemcpyDeviceToHost, ctx_->stream));
        }
        VKX_HIP(hipStreamSynchronize(ctx_->stream));
        return VKX_OK;
    }

private:
    struct Plane {
        const void *in;
        void *out;
        size_t row_bytes;
        int rows;
        ptrdiff_t pitch;
        size_t off;
    };
    vkx_ctx *ctx_;
    std::vector<Plane> planes_;
    size_t total_ = 0;
    bool bad_pitch_ = false;
    vkx_tables mapped_;           // the block of commit_mapped(), and its hold on the ring
    uint8_t *base_ = nullptr;
};

// One host plane of a call: `rows` rows of `row` elements of T, `stride` elements apart in the caller's memory (vkx.h: unused
// with a single row).  On the device the plane is dense: after staging `dev` points to it and `pitch` (== row, in elements, the
// unit the _dev forms take) is its row pitch.  A plane whose pointer is NULL (an optional one) is not staged and keeps dev == NULL.
struct vkx_host_plane_raw {
    const void *in = nullptr;      // read before the call ...
    void *out = nullptr;           // ... written back after it (both: in place)
    size_t row_bytes = 0;
    int rows = 0;
    ptrdiff_t host_pitch = 0;      // bytes
    void *dev_ = nullptr;
};
template <class T> struct vkx_host_plane : vkx_host_plane_raw {
    ptrdiff_t pitch = 0;
    T *dev() const { return (T *)dev_; }
};
template <class T> vkx_host_plane<T> vkx_plane(const T *in, T *out, int rows, size_t w, int cn, ptrdiff_t stride)
{
    vkx_host_plane<T> p;
    p.in = in; p.out = out; p.rows = rows;
    p.pitch = (ptrdiff_t)(w * (size_t)cn);
    p.row_bytes = (size_t)p.pitch * sizeof(T);
    p.host_pitch = stride * (ptrdiff_t)sizeof(T);
    return p;
}
// [rows, w, cn] of T (uint8_t, int16_t, int32_t, int64_t, float, double: deduced from the pointer), stride in elements
template <class T> vkx_host_plane<T> vkx_in(const T *p, int rows, size_t w, int cn, ptrdiff_t stride) { return vkx_plane<T>(p, nullptr, rows, w, cn, stride); }
template <class T> vkx_host_plane<T> vkx_out(T *p, int rows, size_t w, int cn, ptrdiff_t stride) { return vkx_plane<T>(nullptr, p, rows, w, cn, stride); }
template <class T> vkx_host_plane<T> vkx_inout(T *p, int rows, size_t w, int cn, ptrdiff_t stride) { return vkx_plane<T>(p, p, rows, w, cn, stride); }

// A host entry point: stage `planes`, run `dev_call` (the _dev form on their dev() / pitch; int()), copy the outputs back and
// synchronise.  A plane with a short or negative pitch refuses the call (VKX_ERR_INVALID) before anything is moved.
template <class Call> int vkx_host_run(vkx_ctx *ctx, vkx_host_plane_raw *const *planes, size_t n_planes, Call &&dev_call)
{
    HostStage st(ctx);
    std::vector<int> id(n_planes, -1);
    for (size_t i = 0; i < n_planes; i++) {
        const vkx_host_plane_raw &p = *planes[i];
        if (p.in || p.out) id[i] = st.add(p.in, p.out, p.row_bytes, p.rows, p.host_pitch);
    }
    int rc = st.commit();
    if (rc) return rc;
    for (size_t i = 0; i < n_planes; i++) planes[i]->dev_ = st.dev<void>(id[i]);
    if ((rc = dev_call())) return rc;
    return st.finish();
}
template <class Call> int vkx_host_run(vkx_ctx *ctx, std::initializer_list<vkx_host_plane_raw *> planes, Call &&dev_call)
{
    return vkx_host_run(ctx, planes.begin(), planes.size(), dev_call);
}
