// imageencoder_amd/csrc/ie_capi_vdec.cpp -- the streamed video decode of the C ABI (ie_vdec_*): the
// mirror of ie_vstream.  ie_decode_gop reserves a pixel buffer for the whole video and copies the
// frames out after the last one has decoded; here the video flows through two device slots of
// chunk_frames frames each, and the frames of chunk k leave (D2H on a stream of their own, or D2D)
// while chunk k+1 decodes:
//
//   c->stream  | chunk 0 -> slot 0 | chunk 1 -> slot 1 |     | chunk 2 -> slot 0 |   | chunk 3 -> slot 1 |
//   ev_dec     |                  [0]                 [1]                       [0]                     [1]
//   d2h        |                   | frames of chunk 0 |[ev_d2h 0]| frames of chunk 1 |[ev_d2h 1]| ...
//   host       | open .............. next: wait ev_dec[0], read pos, copy, wait ev_d2h[0], enqueue 2 ...
//
// One bit-contiguous chain (VideoDecoder.cpp:28-58, Frame.cpp:47-127) followed chunk by chunk on
// the device: a chunk's first bit is the end bit the chunk before it wrote (gop_cont_kernel reads
// it there), so the host never waits for a decode before it enqueues the next one.  The host waits
// once per chunk, for the chunk's positions and record totals (pinned h_pos), which say how many of
// its frames are whole.
//   gop <= 1: a chunk is ONE exact parse of its frames (DecArgs::nframes = the chunk's frames, the
//             span their bound) from the device start word.
//   gop > 1:  the per-frame launch sequence of ie_decode_gop; a P-frame that opens a chunk reads
//             its reference from the last frame of the other slot.
// What the decoder owns, so that other calls on the context between two ie_vdec_next calls change
// nothing: the stream (a copy, or the caller's 16-byte aligned device stream in place), a device
// copy of the context's EncTables and the block size as they were at open, the position words, the
// two slots, and with motioncomp == 0 the frame of scratch the unapplied error is decoded into.
// The parse scratch (d_rtab, d_rpos, d_walk) stays the context's: it is live only inside one
// chunk's launches, every call on the context is ordered on its stream behind them, and a call that
// regrows it waits for the stream first (Buf::reserve) -- so it is carved again for every chunk.
#include "ie_ctx.hpp"

#include <memory>

using namespace iec;

struct ie_vdec {
    ie_ctx* c = nullptr;
    Stream d2h;  // (first: destroyed after the events and buffers below)
    Event ev_in, ev_dec[2], ev_d2h[2];
    int n = 0, w = 0, h = 0, nframes = 0, gop = 1, merange = 0, mv = 0, rle = 1, motioncomp = 1;
    int K = 1;                       // frames per chunk
    int Ka = 1;                      // frames a slot holds: min(K, nframes)
    int nchunks = 0;                 // ceil(nframes / K)
    uint64_t start_bit = 0, nbits = 0;
    const uint8_t* words = nullptr;  // the stream the kernels read: d_stream, or the caller's in place
    Buf<uint8_t> d_stream;
    Buf<ie::EncTables> d_tab;
    Buf<uint8_t> d_slot[2];          // [Ka] frames, rows w apart, frames w * h apart
    Buf<int16_t> d_err;              // motioncomp == 0: the prediction error nobody applies
    Buf<uint64_t> d_pos;             // [2][2 Ka + 1]: per slot pos[0 .. np] first bits (pos[i + 1] = step i's
                                     // end), then tot[0 .. np) records on each step's true path
    Buf<uint64_t, Mem::Pinned> h_pos;  // its read-back, per slot
    Buf<uint8_t, Mem::Pinned> h_stage; // [Ka] frames on their way to pageable memory
    int enq = 0, deliv = 0;          // chunks enqueued / delivered
    int cur = 0;                     // frames of chunk `deliv` handed out
    int valid = -1;                  // its whole frames; -1: positions not read yet
    int frames_out = 0;
    uint64_t chunk_end = 0;          // the end bit of chunk `deliv` (meaningful when all its frames are whole)
    uint64_t end_bit = UINT64_MAX;   // the video's, once its last frame is out
    std::string bad;                 // non-empty: the stream ended early; what every later next reports
    std::string bad_next;            // the message once the whole frames of chunk `deliv` are out

    size_t fbytes() const { return size_t(w) * size_t(h); }
    int chunk_frames_of(int k) const { return std::min(K, nframes - k * K); }
    int steps_of(int k) const { return gop > 1 ? chunk_frames_of(k) : 1; }  // device-chained launch sets
    size_t pos_words() const { return 2 * size_t(Ka) + 1; }
    ~ie_vdec() {
        if (d2h) (void)hipStreamSynchronize(d2h);
    }
};

namespace {

// The launches of chunk k into slot k & 1, its positions' read-back and its event; no synchronisation.
int vd_enqueue(ie_vdec* v, int k) {
    ie_ctx* c = v->c;
    const int s = k & 1, n = v->n, nf = v->chunk_frames_of(k), np = v->steps_of(k);
    uint64_t* pos = v->d_pos + size_t(s) * v->pos_words();
    uint64_t* tot = pos + np + 1;
    if (k == 0) {
        ie::launch_gop_init(pos, tot, np, v->start_bit, c->stream);
    } else {  // (the chunk before this one is a whole one: K frames)
        const uint64_t* prev = v->d_pos + size_t(s ^ 1) * v->pos_words();
        ie::launch_gop_continue(pos, tot, np, prev + v->steps_of(k - 1), c->stream);
    }
    HIPCHK(c, hipGetLastError());
    const uint64_t nblocks = uint64_t(v->w / n) * (v->h / n);
    const uint64_t rec_bound = nblocks * bound_bits_per_block(n);
    const uint64_t nmb = uint64_t(v->w / 16) * (v->h / 16), mvb = nmb * 2u * uint64_t(v->mv);
    const size_t fb = v->fbytes();
    // the plan of ie_decode_gop for a frame (gop > 1), or of the chunk's frames as one span; the
    // scratch is carved on every chunk (a call between two chunks may have grown it)
    const int pf = v->gop > 1 ? 1 : nf;  // frames per parse
    const uint64_t min_rec = v->rle ? 4u : uint64_t(4 + n * n);
    const uint64_t cmax = v->gop > 1 ? uint64_t(ie::kRecPosCap) * min_rec : kMaxChunkBits;
    RecPlan pl{};
    ie::RecParseArgs pa{};
    int r;
    if ((r = plan_chunks(c, n, uint64_t(pf) * rec_bound, uint64_t(pf) * nblocks, cmax, &pl))) return r;
    if ((r = dec_scratch(c, n, pl, 1, pa))) return r;
    ie::DecArgs da{};
    da.bx = v->w / n;
    da.by = v->h / n;
    da.rle = v->rle;
    da.stride = uint64_t(v->w);
    da.frame_pitch = uint64_t(fb);
    da.tab = v->d_tab;
    da.nframes = pf;
    pa.words = reinterpret_cast<const uint32_t*>(v->words);
    pa.nbits = v->nbits;
    pa.rle = v->rle;
    pa.span = uint64_t(pf) * rec_bound;
    uint8_t* slot = v->d_slot[s];
    for (int i = 0; i < np; i++) {
        uint8_t* fo = slot + size_t(i) * fb;
        const bool iframe = v->gop <= 1 || ((k * v->K + i) % v->gop) == 0;
        if (!iframe) {
            const uint8_t* ref = i ? fo - fb : v->d_slot[s ^ 1] + size_t(v->K - 1) * fb;
            ie::launch_pframe_mvcopy(v->words, 0, pos + i, v->nbits, v->mv, ref, uint64_t(v->w), fo, uint64_t(v->w), v->w,
                                     v->h, c->stream);
            HIPCHK(c, hipGetLastError());
        }
        const bool apply = iframe || v->motioncomp;
        da.out = apply ? fo : reinterpret_cast<uint8_t*>(v->d_err.get());
        da.add_base = (apply && !iframe) ? 1 : 0;
        pa.dstart = pos + i;
        pa.start_add = iframe ? 0 : mvb;
        pa.total = tot + i;
        pa.end_out = pos + i + 1;
        if (ie::launch_rec_parse_decode(pa, da, n, c->stream) < 0)
            return fail(c, IE_EINVAL, "stream too long for one decode call");
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipMemcpyAsync(v->h_pos + size_t(s) * v->pos_words(), pos, (2 * size_t(np) + 1) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(v->ev_dec[s], c->stream));
    v->enq = k + 1;  // (ie_last_decode_info keeps describing the last whole-call decode)
    return IE_OK;
}

// The chunk's one synchronisation: its positions and totals, and from them its whole frames.
int vd_harvest(ie_vdec* v) {
    ie_ctx* c = v->c;
    const int k = v->deliv, s = k & 1, n = v->n, nf = v->chunk_frames_of(k), np = v->steps_of(k);
    HIPCHK(c, hipEventSynchronize(v->ev_dec[s]));
    const uint64_t* hp = v->h_pos + size_t(s) * v->pos_words();
    const uint64_t* ht = hp + np + 1;
    const uint64_t nblocks = uint64_t(v->w / n) * (v->h / n);
    const uint64_t mvb = uint64_t(v->w / 16) * (v->h / 16) * 2u * uint64_t(v->mv);
    v->valid = nf;
    v->bad_next.clear();
    if (v->gop > 1) {  // ie_decode_gop's checks, frame by frame
        for (int i = 0; i < nf && v->bad_next.empty(); i++) {
            if (((k * v->K + i) % v->gop) != 0 && hp[i] + mvb > v->nbits) v->bad_next = "stream ends in the motion vectors";
            else if (ht[i] < nblocks || hp[i + 1] > v->nbits) v->bad_next = "stream ends before the last block";
            if (!v->bad_next.empty()) v->valid = i;
        }
    } else if (ht[0] < uint64_t(nf) * nblocks || hp[1] > v->nbits) {
        // one parse for the chunk: the records counted say how many frames are whole (a record
        // that starts inside the stream is counted even when it runs past its end; the last
        // frame's end is the one the kernels report)
        v->valid = int(std::min<uint64_t>(ht[0] / nblocks, uint64_t(nf - 1)));
        v->bad_next = "stream ends before the last block";
    }
    v->chunk_end = hp[np];
    return IE_OK;
}

// Frames [f0, f0 + nf) of slot s to the caller's out (frame i at out + i * frame_pitch).  A device
// out: copies on the context's stream (the next use of the slot follows in stream order).  A host
// out: on the D2H stream, directly when page-locked, through h_stage otherwise; *pending says that
// ev_d2h[s] must be waited for.
int vd_copy_out(ie_vdec* v, int s, int f0, int nf, uint8_t* out, size_t stride, size_t frame_pitch, bool out_dev,
                bool out_pinned, bool* pending) {
    ie_ctx* c = v->c;
    const size_t fb = v->fbytes(), w = size_t(v->w), h = size_t(v->h);
    const uint8_t* src = v->d_slot[s] + size_t(f0) * fb;
    const bool tight = stride == w && (nf == 1 || frame_pitch == fb);
    if (out_dev || out_pinned) {
        const hipMemcpyKind kind = out_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        hipStream_t st = out_dev ? c->stream : v->d2h.s;
        if (tight) {
            HIPCHK(c, hipMemcpyAsync(out, src, size_t(nf) * fb, kind, st));
        } else {
            for (int i = 0; i < nf; i++)
                HIPCHK(c, hipMemcpy2DAsync(out + size_t(i) * frame_pitch, stride, src + size_t(i) * fb, w, w, h, kind, st));
        }
        if (!out_dev) {
            HIPCHK(c, hipEventRecord(v->ev_d2h[s], v->d2h));
            *pending = true;
        }
        return IE_OK;
    }
    // pageable: one DMA into the pinned staging, then the rows (only the w bytes of each are the decoder's)
    HIPCHK(c, hipMemcpyAsync(v->h_stage, src, size_t(nf) * fb, hipMemcpyDeviceToHost, v->d2h));
    HIPCHK(c, hipEventRecord(v->ev_d2h[s], v->d2h));
    HIPCHK(c, hipEventSynchronize(v->ev_d2h[s]));
    if (tight) {
        std::memcpy(out, v->h_stage, size_t(nf) * fb);
    } else {
        for (int i = 0; i < nf; i++)
            for (size_t r = 0; r < h; r++)
                std::memcpy(out + size_t(i) * frame_pitch + r * stride, v->h_stage + size_t(i) * fb + r * w, w);
    }
    return IE_OK;
}

}  // namespace

extern "C" {

int ie_vdec_open(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes, int gop,
                 int merange, int use_rle, int motioncomp, int chunk_frames, ie_vdec** out) {
    if (!c || !in || !out) return IE_EINVAL;
    *out = nullptr;
    int r = check_dims(c, w, h, nframes);
    if (r) return r;
    gop = std::max(1, gop);
    if (merange < 0 || merange > 32767) return fail(c, IE_EINVAL, "merange must be in [0, 32767]");
    if (gop > 1 && nframes > 1 && (w % 16 || h % 16))
        return fail(c, IE_EINVAL, "P-frames decode for W and H multiples of 16 only: the reference's macroblocks are "
                                  "misplaced otherwise and its uncovered microblocks read records never written");
    if (start_bit > uint64_t(len) * 8) return fail(c, IE_EINVAL, "start_bit beyond the stream");
    if (chunk_frames < 0) return fail(c, IE_EINVAL, "chunk_frames must be >= 0");
    if (c->vdec) return fail(c, IE_EINVAL, "a streamed video decoder is already open on this context");
    HIPCHK(c, hipSetDevice(c->device));
    std::unique_ptr<ie_vdec> v(new ie_vdec());
    v->c = c;
    v->n = c->n;
    v->w = w;
    v->h = h;
    v->nframes = nframes;
    v->gop = gop;
    v->merange = merange;
    v->mv = mvec_bits(merange);
    v->rle = use_rle ? 1 : 0;
    v->motioncomp = motioncomp ? 1 : 0;
    v->start_bit = start_bit;
    v->nbits = uint64_t(len) * 8;
    const size_t fb = v->fbytes();
    v->K = chunk_frames ? chunk_frames : int(std::min<size_t>(std::max<size_t>(1, chunk_target() / fb), size_t(INT32_MAX)));
    v->Ka = std::min(v->K, nframes);
    v->nchunks = (nframes + v->K - 1) / v->K;
    if ((r = v->d2h.create(c, hipStreamNonBlocking)) || (r = v->ev_in.create(c, hipEventDisableTiming))) return r;
    for (int s = 0; s < 2; s++)
        if ((r = v->ev_dec[s].create(c, hipEventDisableTiming)) || (r = v->ev_d2h[s].create(c, hipEventDisableTiming)))
            return r;
    // (Wait::None: nothing enqueued uses these buffers yet -- they are new)
    for (int s = 0; s < std::min(2, v->nchunks); s++)
        if ((r = v->d_slot[s].reserve(c, size_t(v->Ka) * fb, Wait::None))) return r;
    if ((r = v->d_tab.reserve(c, 1, Wait::None)) || (r = v->d_pos.reserve(c, 2 * v->pos_words(), Wait::None)) ||
        (r = v->h_pos.reserve(c, 2 * v->pos_words(), Wait::None)))
        return r;
    if (gop > 1 && nframes > 1 && !motioncomp && (r = v->d_err.reserve(c, (fb + 1) / 2, Wait::None))) return r;
    // the stream as the kernels read it (stage_stream_in's layout): whole aligned words up to the
    // one holding the last byte, then zeros, 16 bytes of padding for the vector loads.  A 16-byte
    // aligned device stream is read in place; anything else is copied now.
    const bool in_dev = is_device_ptr(in);
    v->words = in;
    if (!in_dev || (reinterpret_cast<uintptr_t>(in) & 15u)) {
        const size_t padded = (len + 3) / 4 * 4 + 16;
        if ((r = v->d_stream.reserve(c, padded, Wait::None))) return r;
        HIPCHK(c, hipMemsetAsync(v->d_stream + (len / 4) * 4, 0, padded - (len / 4) * 4, c->stream));
        if (len)
            HIPCHK(c, hipMemcpyAsync(v->d_stream, in, len, in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                     c->stream));
        v->words = v->d_stream;
    }
    HIPCHK(c, hipMemcpyAsync(v->d_tab, c->d_tab, sizeof(ie::EncTables), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipEventRecord(v->ev_in, c->stream));
    for (int k = 0; k < std::min(2, v->nchunks); k++)
        if ((r = vd_enqueue(v.get(), k))) {
            (void)hipStreamSynchronize(c->stream);  // (what was enqueued uses the buffers freed on return)
            return r;
        }
    // the caller's stream and the context's tables are the decoder's own from here on
    HIPCHK(c, hipEventSynchronize(v->ev_in));
    c->vdec = v.get();
    *out = v.release();
    return IE_OK;
}

int ie_vdec_next(ie_vdec* v, uint8_t* out, size_t stride, size_t frame_pitch, int max_frames, int* got) {
    if (!v || !got) return IE_EINVAL;
    ie_ctx* c = v->c;
    *got = 0;
    if (!out) return fail(c, IE_EINVAL, "ie_vdec_next: null out");
    if (max_frames < 1) return fail(c, IE_EINVAL, "max_frames must be >= 1");
    if (stride < size_t(v->w)) return fail(c, IE_EINVAL, "stride < width");
    if (max_frames > 1 && frame_pitch < frames_span(1, 0, stride, v->w, v->h))
        return fail(c, IE_EINVAL, "frame_pitch smaller than a frame");
    if (!v->bad.empty()) return fail(c, IE_EFORMAT, v->bad);
    HIPCHK(c, hipSetDevice(c->device));
    const bool out_dev = is_device_ptr(out), out_pinned = !out_dev && is_pinned_ptr(out);
    if (!out_dev && !out_pinned) {
        int r = v->h_stage.reserve(c, size_t(v->Ka) * v->fbytes(), Wait::None);
        if (r) return r;
    }
    int r = IE_OK;
    int waiting = -1;  // slot whose ev_d2h covers copies of this call not waited for yet
    auto wait_d2h = [&]() -> int {
        if (waiting >= 0) HIPCHK(c, hipEventSynchronize(v->ev_d2h[waiting]));
        waiting = -1;
        return IE_OK;
    };
    while (*got < max_frames && v->frames_out < v->nframes) {
        const int k = v->deliv, s = k & 1, nf = v->chunk_frames_of(k);
        if (v->valid < 0 && (r = vd_harvest(v))) break;
        if (v->cur == v->valid && v->valid < nf) {  // the stream ends inside the next frame
            v->bad = v->bad_next;
            break;
        }
        const int take = std::min(max_frames - *got, v->valid - v->cur);
        bool pending = false;
        if ((r = vd_copy_out(v, s, v->cur, take, out + size_t(*got) * frame_pitch, stride, frame_pitch, out_dev, out_pinned,
                             &pending)))
            break;
        if (pending) waiting = s;
        v->cur += take;
        v->frames_out += take;
        *got += take;
        if (v->cur == nf) {
            // chunk k is out of slot s once its D2H is complete (a device out: in stream order): chunk
            // k + 2 goes in, before this call waits for anything further
            if ((r = wait_d2h())) break;
            if (k == v->nchunks - 1) v->end_bit = v->chunk_end;
            v->deliv = k + 1;
            v->cur = 0;
            v->valid = -1;
            if (v->enq < v->nchunks && (r = vd_enqueue(v, v->enq))) break;
        }
    }
    const int rw = wait_d2h();  // a host out is filled when the call returns
    if (r) return r;
    if (rw) return rw;
    if (!v->bad.empty()) return fail(c, IE_EFORMAT, v->bad);
    return IE_OK;
}

int ie_vdec_info(const ie_vdec* v, int* chunk_frames, int* chunks_enqueued, int* chunks_delivered, uint64_t* end_bit) {
    if (!v) return IE_EINVAL;
    if (chunk_frames) *chunk_frames = v->K;
    if (chunks_enqueued) *chunks_enqueued = v->enq;
    if (chunks_delivered) *chunks_delivered = v->deliv;
    if (end_bit) *end_bit = v->end_bit;
    return IE_OK;
}

int ie_vdec_close(ie_vdec* v) {
    if (!v) return IE_OK;
    ie_ctx* c = v->c;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);  // chunks still decoding into the slots
    if (c->vdec == v) c->vdec = nullptr;
    delete v;  // (~ie_vdec waits for the D2H stream first)
    return IE_OK;
}

}  // extern "C"
