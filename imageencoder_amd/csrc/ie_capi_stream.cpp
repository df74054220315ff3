// imageencoder_amd/csrc/ie_capi_stream.cpp -- the streamed host path of the C ABI (ie_vstream_*,
// and ie_encode_frames / ie_encode_images when frames and streams are both in host memory).
// Host frames in, host streams out (the reference reads and writes whole files, utils.hpp:352-402,
// VideoBase.cpp:6-19): the batch flows through the device in sub-batches ("chunks") of a few
// frames.  Three HIP streams -- H2D (c->pipe->h2d), encode (c->stream), D2H (c->pipe->d2h) --
// with two device slots and two pinned host slots per direction: the H2D of chunk k+1, the encode
// of chunk k and the D2H of chunk k-1 run at the same time (PCIe is full duplex).  Pinned caller
// buffers (ie_host_alloc / hipHostMalloc / hipHostRegister) are DMA'd directly; pageable ones go
// through the pinned slots with a multi-threaded host copy.
#include "ie_ctx.hpp"

#include <atomic>
#include <memory>
#include <mutex>
#include <thread>

using namespace iec;

// The slot buffers are resized with Wait::None: a slot is only resized when nothing of this run
// uses it yet, and later chunks may still be encoding on the context's stream.
struct ie_pipe {
    Stream h2d, d2h;  // (first: destroyed after the events and buffers below)
    Event ev_h2d[2], ev_enc[2], ev_d2h[2];
    bool rec_enc[2] = {}, rec_d2h[2] = {}, rec_h2d[2] = {};
    Buf<uint8_t> d_in[2], d_out[2];
    Buf<uint8_t, Mem::Pinned> h_in[2], h_out[2];
    Buf<uint64_t, Mem::Pinned> h_ends;  // [2][kMaxChunk + 1]: images: each image's chain end;
                                        // video chunks: the frame starts, then [kMaxChunk] the chain end
    Buf<uint32_t, Mem::Pinned> h_hdr;   // [2][kMaxChunk] header words (the word holding start_bit)
    Buf<uint64_t> d_ends;               // [2]: chained launches read the previous end here
    ~ie_pipe() {
        if (h2d) (void)hipStreamSynchronize(h2d);
        if (d2h) (void)hipStreamSynchronize(d2h);
    }
};

// ---- streamed video (ie_vstream_*) ----------------------------------------------------------
// One bit-contiguous chain (Frame.cpp:31-45, VideoEncoder.cpp:83-91) grown chunk by chunk on the
// device: chunk k's launch starts at chunk k-1's chain end read on the device (start_dev), so the
// host never waits for an encode before launching the next; the finished bytes leave through the
// D2H stream while later chunks encode.
// With P-frames (gop > 1, ie_vstream_open_gop) a chunk is K / gop whole groups of pictures and its
// launches are one wave of ie_encode_gop_groups (launch_gop_wave) whose splice starts at the
// previous chunk's end bit in d_pos.  Frames gather in the current input slot across pushes until
// it holds a chunk; finish launches what is left.  The table is the stream's own, not the
// context's d_gop_pos: an ie_encode_gop between two pushes would overwrite the end bit the next
// chunk starts from.  The group scratch is the context's (d_gopg): it is live only inside one
// chunk's launches, all enqueued by one call in stream order.
struct ie_vstream {
    ie_ctx* c = nullptr;
    int w = 0, h = 0, rle = 1, mode = IE_MODE_FAST;
    int gop = 1, merange = 0;
    int fill = 0;                    // gop > 1: frames in the current input slot, not launched yet
    Buf<uint64_t> d_pos;             // gop > 1: [max_frames + 1] first bit of every launched frame; a
                                     // chunk's end bit lies where the next chunk's first frame goes
    Buf<uint64_t, Mem::Pinned> h_pos;  // gop > 1: [2][K + 1] read-back of a chunk's part of d_pos
    size_t stride = 0, frame_pitch = 0;
    uint64_t start_bit = 0;
    int max_frames = 0, frames = 0;  // capacity, frames launched
    int K = 1;                       // frames per chunk
    Buf<uint8_t> d_stream;           // the whole stream from byte 0 (the caller's head included)
    int chunks = 0;                  // chunks launched
    int harvested = 0;               // chunks whose frame starts / end are known on the host
    uint64_t done_bits = 0;          // chain end of the last harvested chunk
    uint64_t pulled = 0;             // bytes [0, pulled) handed out by ie_vstream_pull
    int chunk_f0[2] = {}, chunk_nf[2] = {};
    std::vector<uint64_t> fs;        // absolute start bit of every harvested frame
    ie_pipe P;                       // its own streams, events and slots (last: its streams are
                                     // synchronised before anything above is freed)
};

namespace {

// memcpy split over a few threads (a single core copies ~10 GB/s, PCIe moves ~50 GB/s).
void par_copy(uint8_t* dst, const uint8_t* src, size_t n) {
    constexpr size_t kPart = size_t(4) << 20;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t parts = std::min<size_t>(std::min<size_t>(hw, 8), (n + kPart - 1) / kPart);
    if (parts <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t per = (n + parts - 1) / parts;
    std::vector<std::thread> th;
    th.reserve(parts - 1);
    for (size_t i = 1; i < parts; i++) {
        const size_t b = i * per, e = std::min(n, b + per);
        if (b < e) th.emplace_back([=] { std::memcpy(dst + b, src + b, e - b); });
    }
    std::memcpy(dst, src, std::min(n, per));
    for (auto& t : th) t.join();
}

using Pipe = ie_pipe;
constexpr int kMaxChunk = 64;

int pipe_init(ie_ctx* c, Pipe* P) {
    int r;
    if ((r = P->h2d.create(c, hipStreamNonBlocking)) || (r = P->d2h.create(c, hipStreamNonBlocking))) return r;
    for (int i = 0; i < 2; i++)
        if ((r = P->ev_h2d[i].create(c, hipEventDisableTiming)) || (r = P->ev_enc[i].create(c, hipEventDisableTiming)) ||
            (r = P->ev_d2h[i].create(c, hipEventDisableTiming)))
            return r;
    if ((r = P->h_ends.reserve(c, 2 * (kMaxChunk + 1))) || (r = P->h_hdr.reserve(c, 2 * kMaxChunk))) return r;
    return P->d_ends.reserve(c, 2);
}

// The context's pipeline for streamed image batches; a new run starts with nothing pending (the
// previous one ended with a full synchronisation).
int pipe_get(ie_ctx* c, Pipe*& P) {
    if (!c->pipe) {
        c->pipe = new Pipe();
        int r = pipe_init(c, c->pipe);
        if (r) {
            pipe_free(c->pipe);
            c->pipe = nullptr;
            return r;
        }
    }
    P = c->pipe;
    for (int i = 0; i < 2; i++) P->rec_enc[i] = P->rec_d2h[i] = P->rec_h2d[i] = false;
    return IE_OK;
}

// frames per chunk: ~8 MiB of pixels (at least 1, at most kMaxChunk), and at least two chunks
// (IE_CHUNK_MB overrides the target: a tuning aid, the output does not depend on it)
int chunk_frames(size_t frame_bytes, int nframes) {
    int k = int(std::max<size_t>(1, chunk_target() / std::max<size_t>(1, frame_bytes)));
    k = std::min(k, kMaxChunk);
    k = std::min(k, (nframes + 1) / 2);
    return std::max(k, 1);
}

// Upload chunk `k` (frames f0 .. f0+nf-1) into device slot s, from byte `at` of it on, on the H2D stream.
int pipe_upload(ie_ctx* c, Pipe* P, int s, const uint8_t* y, size_t frame_pitch, size_t in_bytes, int f0,
                bool pinned_in, size_t at = 0) {
    // d_in[s] is free once the encode of the chunk that last used it is done
    if (P->rec_enc[s]) HIPCHK(c, hipStreamWaitEvent(P->h2d, P->ev_enc[s], 0));
    const uint8_t* src = y + size_t(f0) * frame_pitch;
    if (pinned_in) {
        HIPCHK(c, hipMemcpyAsync(P->d_in[s] + at, src, in_bytes, hipMemcpyHostToDevice, P->h2d));
    } else {
        if (P->rec_h2d[s]) HIPCHK(c, hipEventSynchronize(P->ev_h2d[s]));  // h_in[s] drained
        par_copy(P->h_in[s] + at, src, in_bytes);
        HIPCHK(c, hipMemcpyAsync(P->d_in[s] + at, P->h_in[s] + at, in_bytes, hipMemcpyHostToDevice, P->h2d));
    }
    HIPCHK(c, hipEventRecord(P->ev_h2d[s], P->h2d));
    P->rec_h2d[s] = true;
    return IE_OK;
}

// The host side of chunk j (the oldest unharvested one): its frame starts and chain end.
int vs_harvest(ie_vstream* v) {
    ie_ctx* c = v->c;
    Pipe* P = &v->P;
    const int j = v->harvested, s = j & 1;
    HIPCHK(c, hipEventSynchronize(P->ev_enc[s]));
    const uint64_t* hs = v->gop > 1 ? v->h_pos + size_t(s) * size_t(v->K + 1) : P->h_ends + s * (kMaxChunk + 1);
    for (int i = 0; i < v->chunk_nf[s]; i++) v->fs[size_t(v->chunk_f0[s] + i)] = hs[i];
    v->done_bits = hs[v->gop > 1 ? v->chunk_nf[s] : kMaxChunk];
    v->harvested = j + 1;
    return IE_OK;
}

// One chunk: upload, then a launch continuing the chain on the device.
int vs_chunk(ie_vstream* v, const uint8_t* frames, int nf, bool pinned_in) {
    ie_ctx* c = v->c;
    Pipe* P = &v->P;
    const int k = v->chunks, s = k & 1;
    while (k - v->harvested >= 2) {  // slot s's read-back area still holds chunk k-2's ends
        int r = vs_harvest(v);
        if (r) return r;
    }
    const size_t ib = frames_span(nf, v->frame_pitch, v->stride, v->w, v->h);
    int r;
    if ((r = pipe_upload(c, P, s, frames, v->frame_pitch, ib, 0, pinned_in))) return r;
    HIPCHK(c, hipStreamWaitEvent(c->stream, P->ev_h2d[s], 0));
    Launch L(P->d_in[s], v->w, v->h, v->stride, v->frame_pitch, nf, v->rle, v->mode,
             reinterpret_cast<uint32_t*>(v->d_stream.get()), v->start_bit);
    L.start_dev = k ? P->d_ends + ((k - 1) & 1) : nullptr;
    L.chain_end = P->d_ends + s;
    if ((r = launch_chain(c, L))) return r;
    uint64_t* hs = P->h_ends + s * (kMaxChunk + 1);
    HIPCHK(c, hipMemcpyAsync(hs, c->d_frame_start, size_t(nf) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hs + kMaxChunk, P->d_ends + s, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(P->ev_enc[s], c->stream));
    P->rec_enc[s] = true;
    note_async(c, "streamed video encode");
    v->chunk_f0[s] = v->frames;
    v->chunk_nf[s] = nf;
    v->frames += nf;
    v->chunks = k + 1;
    return IE_OK;
}

// gop > 1: launch the v->fill frames gathered in the current input slot as one wave of groups.
int vs_gop_launch(ie_vstream* v) {
    ie_ctx* c = v->c;
    Pipe* P = &v->P;
    const int k = v->chunks, s = k & 1, nfw = v->fill, gw = (nfw + v->gop - 1) / v->gop;
    int r;
    while (k - v->harvested >= 2)  // slot s's read-back area still holds chunk k-2's positions
        if ((r = vs_harvest(v))) return r;
    HIPCHK(c, hipStreamWaitEvent(c->stream, P->ev_h2d[s], 0));
    // (carved on every chunk: a call between two pushes may have grown the context's scratch)
    GopWave W;
    if ((r = gop_wave_scratch(c, v->w, v->h, v->gop, v->merange, size_t(v->K / v->gop), &W))) return r;
    uint64_t* fpos = v->d_pos + v->frames;  // fpos[0] holds the previous chunk's end bit
    if ((r = launch_gop_wave(c, W, P->d_in[s], v->w, v->h, v->stride, v->frame_pitch, gw, nfw, v->merange, v->rle, v->mode,
                             reinterpret_cast<uint32_t*>(v->d_stream.get()), v->start_bit, k ? fpos : nullptr, fpos)))
        return r;
    HIPCHK(c, hipMemcpyAsync(v->h_pos + size_t(s) * size_t(v->K + 1), fpos, size_t(nfw + 1) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(P->ev_enc[s], c->stream));
    P->rec_enc[s] = true;
    note_async(c, "streamed video encode");
    v->chunk_f0[s] = v->frames;
    v->chunk_nf[s] = nfw;
    v->frames += nfw;
    v->fill = 0;
    v->chunks = k + 1;
    return IE_OK;
}

// gop > 1: frames go to the current input slot behind those already there; a full slot is launched.
int vs_gop_push(ie_vstream* v, const uint8_t* frames, int nframes, bool pinned_in) {
    for (int f = 0; f < nframes;) {
        const int s = v->chunks & 1, nf = std::min(v->K - v->fill, nframes - f);
        int r = pipe_upload(v->c, &v->P, s, frames, v->frame_pitch, frames_span(nf, v->frame_pitch, v->stride, v->w, v->h),
                            f, pinned_in, size_t(v->fill) * v->frame_pitch);
        if (r) return r;
        v->fill += nf;
        f += nf;
        if (v->fill == v->K && (r = vs_gop_launch(v))) return r;
    }
    return IE_OK;
}

// Copy stream bytes [v->pulled, b1) to dst (host, pinned or pageable) through the D2H stream:
// pinned destinations directly, pageable ones in 16 MiB pieces through two pinned slots (the
// host copies piece i out while piece i+1 is in flight).
int vs_copy_out(ie_vstream* v, uint8_t* dst, uint64_t b1) {
    ie_ctx* c = v->c;
    Pipe* P = &v->P;
    if (b1 <= v->pulled) return IE_OK;
    const size_t n = size_t(b1 - v->pulled);
    const uint8_t* src = v->d_stream + v->pulled;
    // the bytes were written by the launches up to the last harvested chunk (on c->stream)
    HIPCHK(c, hipStreamWaitEvent(P->d2h, P->ev_enc[(v->harvested - 1) & 1], 0));
    if (is_pinned_ptr(dst)) {
        HIPCHK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, P->d2h));
        HIPCHK(c, hipStreamSynchronize(P->d2h));
    } else {
        constexpr size_t kPiece = size_t(16) << 20;
        int r;
        for (int s = 0; s < 2; s++)
            if ((r = P->h_out[s].reserve(c, std::min(n, kPiece), Wait::None))) return r;
        const size_t pieces = (n + kPiece - 1) / kPiece;
        for (size_t i = 0; i <= pieces; i++) {
            if (i < pieces) {  // slot i&1 was emptied at step i-1
                const size_t o = i * kPiece, len = std::min(kPiece, n - o);
                HIPCHK(c, hipMemcpyAsync(P->h_out[i & 1], src + o, len, hipMemcpyDeviceToHost, P->d2h));
                HIPCHK(c, hipEventRecord(P->ev_d2h[i & 1], P->d2h));
            }
            if (i >= 1) {
                const size_t j = i - 1, o = j * kPiece, len = std::min(kPiece, n - o);
                HIPCHK(c, hipEventSynchronize(P->ev_d2h[j & 1]));
                par_copy(dst + o, P->h_out[j & 1], len);
            }
        }
    }
    v->pulled = b1;
    return IE_OK;
}

// ie_vstream_open (gop = 1) and ie_vstream_open_gop (gop > 1)
int vs_open(ie_ctx* c, int w, int h, size_t stride, size_t frame_pitch, int gop, int merange, int use_rle, int mode,
            const uint8_t* head, uint64_t start_bit, int max_frames, ie_vstream** out) {
    if (!c || !out || max_frames <= 0 || (start_bit && !head)) return IE_EINVAL;
    *out = nullptr;
    // (frames arrive push by push: the pitch must hold a frame even when max_frames is 1)
    int r = check_frames(c, w, h, std::max(max_frames, 2), stride, frame_pitch);
    if (r) return r;
    size_t gop_cap = 0;
    if (gop > 1 && (r = check_gop(c, w, h, stride, frame_pitch, max_frames, gop, merange, SIZE_MAX, start_bit, &gop_cap)))
        return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::unique_ptr<ie_vstream> v(new ie_vstream());
    Pipe* P = &v->P;
    if ((r = pipe_init(c, P))) return r;
    v->c = c;
    v->w = w;
    v->h = h;
    v->stride = stride;
    v->frame_pitch = frame_pitch;
    v->rle = use_rle ? 1 : 0;
    v->mode = mode;
    v->start_bit = start_bit;
    v->max_frames = max_frames;
    v->gop = std::max(gop, 1);
    v->merange = merange;
    if (gop > 1) {
        // a chunk is Gc whole groups: IE_CHUNK_MB's pixel target (no more than the video has), under
        // the ceilings of a wave of ie_encode_gop_groups (gop_wave_groups), at least one group
        const size_t G = (size_t(max_frames) + size_t(gop) - 1) / size_t(gop);
        const size_t want = std::min(G, chunk_target() / std::max<size_t>(1, stride * size_t(h) * size_t(gop)));
        v->K = int(gop_wave_groups(c->n, w, h, gop, merange, want)) * gop;
    } else {
        v->K = chunk_frames(stride * size_t(h), 1 << 20);
    }
    v->fs.assign(size_t(max_frames), 0);
    v->done_bits = start_bit;
    const size_t cap = gop > 1 ? gop_cap : ie_stream_bound(w, h, c->n, max_frames, start_bit);
    const size_t in_bytes = frames_span(v->K, frame_pitch, stride, w, h);
    if ((r = v->d_stream.reserve(c, cap))) return r;
    if (gop > 1 && ((r = v->d_pos.reserve(c, size_t(max_frames) + 1)) || (r = v->h_pos.reserve(c, 2 * size_t(v->K + 1)))))
        return r;
    for (int s = 0; s < 2; s++)
        if ((r = P->d_in[s].reserve(c, in_bytes, Wait::None)) || (r = P->h_in[s].reserve(c, in_bytes, Wait::None))) return r;
    // the caller's head: bytes [0, ceil(start_bit/8)), bits from start_bit on cleared; the word
    // holding start_bit is completed by the first chunk's first tile.  gop > 1: the splice ORs every
    // group's first and last word into the stream, so all of it starts as zeros.
    const size_t hb = size_t((start_bit + 7) / 8);
    std::vector<uint8_t> hd(hb + 8, 0);
    if (hb) std::memcpy(hd.data(), head, hb);
    if (start_bit % 8) hd[hb - 1] &= uint8_t(0xFF00u >> (start_bit % 8));
    if (hipMemsetAsync(v->d_stream, 0, gop > 1 ? cap : std::min(cap, hb + 8), c->stream) != hipSuccess ||
        (hb && hipMemcpyAsync(v->d_stream, hd.data(), hb, hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, IE_EHIP, "video stream head upload");
    *out = v.release();
    return IE_OK;
}

}  // namespace

extern "C" {

int ie_vstream_open(ie_ctx* c, int w, int h, size_t stride, size_t frame_pitch, int use_rle, int mode,
                    const uint8_t* head, uint64_t start_bit, int max_frames, ie_vstream** out) {
    return vs_open(c, w, h, stride, frame_pitch, 1, 0, use_rle, mode, head, start_bit, max_frames, out);
}

int ie_vstream_open_gop(ie_ctx* c, int w, int h, size_t stride, size_t frame_pitch, int gop, int merange, int use_rle,
                        int mode, const uint8_t* head, uint64_t start_bit, int max_frames, ie_vstream** out) {
    if (gop <= 1)
        return ie_vstream_open(c, w, h, stride, frame_pitch, use_rle, mode, head, start_bit, max_frames, out);
    return vs_open(c, w, h, stride, frame_pitch, gop, merange, use_rle, mode, head, start_bit, max_frames, out);
}

int ie_vstream_push(ie_vstream* v, const uint8_t* frames, int nframes) {
    if (!v || (!frames && nframes)) return IE_EINVAL;
    ie_ctx* c = v->c;
    if (nframes < 0 || v->frames + v->fill + nframes > v->max_frames)
        return fail(c, IE_ECAP, "more frames pushed than ie_vstream_open's max_frames");
    if (ie_is_device_ptr(frames)) return fail(c, IE_EINVAL, "ie_vstream_push takes host frames");
    HIPCHK(c, hipSetDevice(c->device));
    // the previous push's pinned frames may still be in flight: they are released now
    HIPCHK(c, hipStreamSynchronize(v->P.h2d));
    const bool pinned = is_pinned_ptr(frames);
    if (v->gop > 1) return vs_gop_push(v, frames, nframes, pinned);
    for (int f = 0; f < nframes; f += v->K) {
        const int r = vs_chunk(v, frames + size_t(f) * v->frame_pitch, std::min(v->K, nframes - f), pinned);
        if (r) return r;
    }
    return IE_OK;
}

int ie_vstream_pull(ie_vstream* v, uint8_t* dst, size_t cap, size_t* nbytes) {
    if (!v || !nbytes || (!dst && cap)) return IE_EINVAL;
    *nbytes = 0;
    // every chunk but the newest is complete or nearly so: harvest them (the newest keeps encoding)
    while (v->harvested < v->chunks - 1) {
        const int r = vs_harvest(v);
        if (r) return r;
    }
    const uint64_t b1 = v->done_bits / 8;  // whole bytes (the partial one follows with the next chunk)
    if (b1 <= v->pulled) return IE_OK;
    if (b1 - v->pulled > cap) return fail(v->c, IE_ECAP, "pull buffer smaller than the finished bytes");
    const uint64_t b0 = v->pulled;
    const int r = vs_copy_out(v, dst, b1);
    if (r) return r;
    *nbytes = size_t(b1 - b0);
    return IE_OK;
}

int ie_vstream_finish(ie_vstream* v, uint8_t* dst, size_t cap, size_t* nbytes, uint64_t* end_bit,
                      uint64_t* frame_bits) {
    if (!v || (!dst && cap)) return IE_EINVAL;
    ie_ctx* c = v->c;
    if (nbytes) *nbytes = 0;
    int r;
    if (v->fill && (r = vs_gop_launch(v))) return r;  // gop > 1: the remainder, its last group maybe short
    while (v->harvested < v->chunks)
        if ((r = vs_harvest(v))) return r;
    unsigned timeouts = 0;
    if ((r = read_errors(c, &timeouts, &c->last_fallbacks))) return r;
    if (timeouts) return lookback_failed(c, " in a streamed video chunk");
    const uint64_t end = v->done_bits, b1 = (end + 7) / 8;
    if (dst) {
        if (b1 - v->pulled > cap) return fail(c, IE_ECAP, "finish buffer smaller than the remaining bytes");
        const uint64_t b0 = v->pulled;
        if ((r = vs_copy_out(v, dst, b1))) return r;
        if (nbytes) *nbytes = size_t(b1 - b0);
    }
    if (end_bit) *end_bit = end;
    if (frame_bits)
        for (int f = 0; f < v->frames; f++)
            frame_bits[f] = ((f + 1 < v->frames) ? v->fs[size_t(f + 1)] : end) - v->fs[size_t(f)];
    return IE_OK;
}

const uint8_t* ie_vstream_device(const ie_vstream* v) { return v ? v->d_stream : nullptr; }

int ie_vstream_close(ie_vstream* v) {
    if (!v) return IE_OK;
    ie_ctx* c = v->c;
    (void)hipStreamSynchronize(c->stream);
    delete v;
    return IE_OK;
}

}  // extern "C"

namespace iec {

size_t chunk_target() {
    const char* e = getenv("IE_CHUNK_MB");
    return (e && atof(e) > 0) ? size_t(atof(e) * 1048576.0) : size_t(8) << 20;
}

void pipe_free(Pipe* p) { delete p; }  // (~ie_pipe waits for its two streams first)

int streamed_images(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                    int use_rle, int mode, uint8_t* out, size_t out_pitch, uint64_t start_bit, uint64_t* end_bits) {
    // Three host threads keep the three streams busy: the uploader issues chunk k's H2D, this
    // thread chunk k's encode, the downloader chunk k's stream D2H.  A copy from or to PAGEABLE
    // memory is synchronous for its calling thread (the runtime stages it), so each direction has
    // its own thread and both PCIe directions stay busy; pinned memory is DMA'd directly.
    Pipe* P;
    int r;
    if ((r = pipe_get(c, P))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int K = chunk_frames(stride * size_t(h), nframes);
    const int nchunks = (nframes + K - 1) / K;
    const size_t in_bytes = frames_span(K, frame_pitch, stride, w, h);
    const uint64_t w0 = start_bit / 32;
    const size_t b0 = size_t(start_bit / 8);
    const size_t stage = out_pitch * size_t(K - 1) + (out_pitch - size_t(w0) * 4);  // slot: from word w0 of image 0
    for (int s = 0; s < 2; s++)
        if ((r = P->d_in[s].reserve(c, in_bytes, Wait::None)) || (r = P->d_out[s].reserve(c, stage, Wait::None))) return r;
    std::vector<uint64_t> ends(size_t(nframes), 0);
    // hand-offs between the three threads: counters of chunks whose H2D / encode / D2H are
    // issued, waited on by spinning (a condition variable's wake-up costs tens of microseconds
    // per hand-off, several per chunk)
    std::atomic<int> uploaded{0}, enqueued{0}, downloaded{0};
    std::atomic<int> err{IE_OK};
    std::mutex mu;
    std::string msg;
    auto set_err = [&](int code, const std::string& m) {
        std::lock_guard<std::mutex> lk(mu);
        int ok = IE_OK;
        if (err.compare_exchange_strong(ok, code)) msg = m;
    };
    auto wait_for = [&](const std::atomic<int>& counter, int value) {  // false: another thread failed
        while (counter.load(std::memory_order_acquire) < value) {
            if (err.load(std::memory_order_relaxed) != IE_OK) return false;
            std::this_thread::yield();
        }
        return err.load(std::memory_order_relaxed) == IE_OK;
    };
    auto publish = [&](std::atomic<int>& counter) { counter.fetch_add(1, std::memory_order_release); };
#define TCHK(expr)                                                                   \
    do {                                                                             \
        hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess) {                                                      \
            set_err(IE_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
            return;                                                                  \
        }                                                                            \
    } while (0)
    // the three roles, per chunk
    auto upload = [&](int k) {
        const int s = k & 1, f0 = k * K, nf = std::min(K, nframes - f0);
        if (!wait_for(enqueued, k - 1)) return;  // d_in[s]'s previous reader (chunk k-2) is launched
        if (k >= 2) TCHK(hipStreamWaitEvent(P->h2d, P->ev_enc[s], 0));
        const size_t ib = frames_span(nf, frame_pitch, stride, w, h);
        TCHK(hipMemcpyAsync(P->d_in[s], y + size_t(f0) * frame_pitch, ib, hipMemcpyHostToDevice, P->h2d));
        TCHK(hipEventRecord(P->ev_h2d[s], P->h2d));
        publish(uploaded);
    };
    auto download = [&](int j) {
        const int s = j & 1, f0 = j * K, nf = std::min(K, nframes - f0);
        if (!wait_for(enqueued, j + 1)) return;
        TCHK(hipEventSynchronize(P->ev_enc[s]));  // its end bits are in h_ends[s] (written by the encoder)
        const uint64_t* he = P->h_ends + s * (kMaxChunk + 1);
        for (int i = 0; i < nf; i++) {
            const uint64_t e = he[i];
            ends[size_t(f0 + i)] = e;
            const size_t n = size_t((e + 7) / 8) - b0;
            const uint8_t* src = P->d_out[s] + size_t(i) * out_pitch + (b0 - size_t(w0) * 4);
            if (n) TCHK(hipMemcpyAsync(out + size_t(f0 + i) * out_pitch + b0, src, n, hipMemcpyDeviceToHost, P->d2h));
        }
        TCHK(hipEventRecord(P->ev_d2h[s], P->d2h));
        publish(downloaded);
    };
    auto encode_chunk = [&](int k) {
        const int s = k & 1, f0 = k * K, nf = std::min(K, nframes - f0);
        // chunk k-2 (slot s) fully out: its streams downloaded (d_out[s]) and its ends read (h_ends[s])
        if (!wait_for(uploaded, k + 1) || !wait_for(downloaded, k - 1)) return;
        TCHK(hipStreamWaitEvent(c->stream, P->ev_h2d[s], 0));
        if (k >= 2) TCHK(hipStreamWaitEvent(c->stream, P->ev_d2h[s], 0));
        // each image's word holding start_bit (the caller's header bits), read by the device from
        // page-locked memory (h_hdr[s] is free: chunk k-2's encode has completed)
        uint32_t* hw = P->h_hdr + s * kMaxChunk;
        for (int i = 0; i < nf; i++) std::memcpy(&hw[i], out + size_t(f0 + i) * out_pitch + size_t(w0) * 4, 4);
        ie::launch_word_scatter(hw, reinterpret_cast<uint32_t*>(P->d_out[s].get()), out_pitch / 4, nf, c->stream);
        Launch L(P->d_in[s], w, h, stride, frame_pitch, nf, use_rle, mode, reinterpret_cast<uint32_t*>(P->d_out[s].get()) - w0,
                 start_bit);
        L.out_pitch = out_pitch;
        L.segmented = 1;
        // each image's end bit goes straight to page-locked host memory (no small SDMA read-back
        // queued behind the stream downloads)
        L.chain_end = P->h_ends + s * (kMaxChunk + 1);
        const int rl = launch_chain(c, L);
        if (rl != IE_OK) return set_err(rl, c->err);
        TCHK(hipEventRecord(P->ev_enc[s], c->stream));
        note_async(c, "streamed encode");
        publish(enqueued);
    };
    if (is_pinned_ptr(y) && is_pinned_ptr(out)) {
        // pinned both ways: every copy is asynchronous, one thread issues everything in order
        for (int k = 0; k < nchunks && err.load() == IE_OK; k++) {
            upload(k);
            encode_chunk(k);
            if (k >= 1) download(k - 1);
        }
        if (err.load() == IE_OK) download(nchunks - 1);
    } else {
        const int dev = c->device;
        std::thread uploader([&] {
            if (hipSetDevice(dev) != hipSuccess) return set_err(IE_EHIP, "hipSetDevice (uploader)");
            for (int k = 0; k < nchunks && err.load() == IE_OK; k++) upload(k);
        });
        std::thread downloader([&] {
            if (hipSetDevice(dev) != hipSuccess) return set_err(IE_EHIP, "hipSetDevice (downloader)");
            for (int j = 0; j < nchunks && err.load() == IE_OK; j++) download(j);
        });
        for (int k = 0; k < nchunks && err.load() == IE_OK; k++) encode_chunk(k);
        uploader.join();
        downloader.join();
    }
#undef TCHK
    (void)hipStreamSynchronize(P->h2d);
    (void)hipStreamSynchronize(P->d2h);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (err.load() != IE_OK) return fail(c, err.load(), msg);
    unsigned timeouts = 0;
    r = read_errors(c, &timeouts, &c->last_fallbacks);
    if (r == IE_EDEVICE || (r == IE_OK && timeouts)) {
        // a look-back timeout in one of this call's own chunks, which ran without tickets
        // (encode() comes here only then; read_errors charges it to them as IE_EDEVICE, so this is
        // not ticket_redo's case): redo the batch through the staged path with ticket-ordered tiles
        c->use_ticket = true;
        return encode(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_pitch * size_t(nframes),
                      out_pitch, start_bit, 1, nullptr, end_bits);
    }
    if (r) return r;
    if (end_bits) std::memcpy(end_bits, ends.data(), ends.size() * sizeof(uint64_t));
    return IE_OK;
}

// ie_encode_frames with host frames and a host stream: the video stream pipeline, pulled into the
// caller's buffer as the chunks finish.
int streamed_frames(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                    int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit, uint64_t* frame_bits,
                    uint64_t* end_bit) {
    ie_vstream* v = nullptr;
    int r = ie_vstream_open(c, w, h, stride, frame_pitch, use_rle, mode, out, start_bit, nframes, &v);
    if (r) return r;
    size_t got = 0;
    for (int f = 0; f < nframes && r == IE_OK; f += v->K) {
        const int nf = std::min(v->K, nframes - f);
        if ((r = ie_vstream_push(v, y + size_t(f) * frame_pitch, nf))) break;
        const uint64_t b0 = v->pulled;
        if ((r = ie_vstream_pull(v, out + b0, out_cap - size_t(b0), &got))) break;
    }
    uint64_t end = 0;
    if (r == IE_OK) {
        const uint64_t b0 = v->pulled;
        r = ie_vstream_finish(v, out + b0, out_cap - size_t(b0), &got, &end, frame_bits);
    }
    ie_vstream_close(v);
    if (r == IE_EDEVICE && !c->use_ticket) {  // a look-back timeout: redo through the staged path
        c->use_ticket = true;
        return encode(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_cap, 0, start_bit, 0,
                      frame_bits, end_bit);
    }
    if (r) return r;
    if (end_bit) *end_bit = end;
    return IE_OK;
}

}  // namespace iec
