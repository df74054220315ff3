// imageencoder_amd/csrc/ie_ctx.hpp -- internal to the C ABI implementation (ie_capi*.cpp,
// ie_tables.cpp): the context, the owners of its memory and handles (Buf, Event, Stream), and the
// checks and staging steps the entry points share.  Functions that cross a file boundary are
// declared here, in namespace iec, and nowhere else.
//
// Every device or pinned allocation of the context, of a streamed pipeline and of a video stream
// is a Buf member: it holds the pointer and the capacity, grows through reserve() and frees itself
// when its owner is deleted.  A new buffer is one member and its reserve() calls; no teardown code
// names it.  Events and side streams are Event / Stream members in the same way.
#pragma once
#include "ie_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "ie_device.h"

// Profiling knobs exist only in IE_PROFILE builds (tools/variants.sh): the product library never
// reads IE_ABLATE / IE_STAMPS / IE_DEC_STAMPS, so no environment variable can change its output.  IE_ABLATE_FORCE: A/B builds of an ablation.
#ifndef IE_PROFILE
#define IE_PROFILE 0
#endif
#ifndef IE_ABLATE_FORCE
#define IE_ABLATE_FORCE 0
#endif

struct ie_pipe;  // streamed host path (ie_capi_stream.cpp)
struct ie_vdec;  // streamed video decode (ie_capi_vdec.cpp)
struct ie_ctx;

namespace iec {
constexpr int kErrWords = 66;  // d_err: [0] look-back timeouts; sum of [2..65] = FP64 re-evaluations

// Device: hipMalloc.  Pinned: hipHostMalloc.  Mapped: pinned memory the device writes directly
// (hipHostMallocMapped | hipHostMallocCoherent); dev() is the device's view of it.
enum class Mem { Device, Pinned, Mapped };
// What reserve() does before it replaces a buffer: wait for the context's stream (work enqueued
// there may still use the old one), or nothing (the caller knows that nothing does).
enum class Wait { Stream, None };

// An owning buffer of `cap()` elements.  Converts to T*, so pointer arithmetic and kernel arguments
// read as with a raw pointer.
template <class T, Mem K = Mem::Device>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { (void)release(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    T* dev() const {
        static_assert(K == Mem::Mapped, "only mapped memory has a device view");
        return dev_;
    }
    size_t cap() const { return cap_; }
    // Room for `elems` elements: at once if there is; otherwise waits as `wait` says, frees, and
    // allocates max(elems, cap + cap / 2).  The contents are not kept.
    int reserve(ie_ctx* c, size_t elems, Wait wait = Wait::Stream);

private:
    hipError_t release() {
        hipError_t e = hipSuccess;
        if (p_) e = K == Mem::Device ? hipFree(p_) : hipHostFree(p_);
        p_ = dev_ = nullptr;
        cap_ = 0;
        return e;
    }
    T* p_ = nullptr;
    T* dev_ = nullptr;
    size_t cap_ = 0;
};

// An event / a stream the owner destroys.  create() is lazy: it does nothing once the handle exists.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
    int create(ie_ctx* c, unsigned flags = hipEventDefault);
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
    int create(ie_ctx* c, unsigned flags);
};
}  // namespace iec

struct ie_ctx {
    int device = 0;
    // (the streams come first: members are destroyed last to first, so every buffer and event
    // below is gone before the streams that used it)
    iec::Stream own;
    iec::Stream tab_stream;
    hipStream_t stream = nullptr;
    std::string err;

    int n = 0;
    uint16_t q[64] = {};
    iec::Buf<ie::EncTables, iec::Mem::Pinned> h_tab;
    iec::Buf<ie::EncTables> d_tab;

    // decoupled look-back state
    iec::Buf<uint64_t> d_state;   // [kStateWordsPerTile * state_tiles()] tile chain granules (ie_common.hpp)
    size_t state_tiles() const { return d_state.cap() / size_t(ie::kStateWordsPerTile); }
    uint32_t tag = 0;
    iec::Buf<unsigned long long> d_ticket;
    unsigned long long ticket_base = 0;

    iec::Buf<uint64_t> d_frame_start;   // [>= 64] grows with d_chain_end
    iec::Buf<uint64_t> d_chain_end;
    iec::Buf<unsigned> d_err;           // [kErrWords] counters that only grow
    iec::Buf<uint32_t> d_wave_fix;      // [state_tiles() * waves per tile] fix-up requests of the last launch
    int last_fix_words = 0;
    unsigned err_seen[iec::kErrWords] = {};  // d_err's values at the previous read
    bool use_ticket = false;            // order tiles with an atomic ticket (after a timeout)
    iec::Event stage_ev[4];             // timing events around the last batched histogram [0,1] / pack [2,3]
    bool stage_rec[2] = {false, false};
    bool stage_timing = false;          // ie_set_stage_timing
    int fake_timeouts = 0;              // debug (IE_FAKE_TIMEOUTS): report this many look-back timeouts
    bool fake_fired = false;            // a faked timeout was reported (the redo paths dirty the output first)
    // Asynchronous launches (no read-back) since the last error read: a look-back timeout found
    // at the next read is charged to them (their output is invalid), never silently retried away.
    unsigned async_pending = 0;
    const char* async_what = nullptr;

    // staging for host-resident inputs / outputs
    iec::Buf<uint8_t> d_in;
    iec::Buf<uint8_t> d_out;
    iec::Buf<uint8_t> d_scratch;    // quantize-only stream sink
    iec::Buf<int16_t> d_coef;

    uint64_t last_fallbacks = 0;

    // Huffman tables / histogram
    iec::Buf<uint32_t> d_code;         // [256] codes, then [256/4] packed lengths (one block)
    iec::Buf<uint32_t, iec::Mem::Pinned> h_code;  // pinned mirror
    iec::Buf<uint32_t> d_hist;         // [256]
    // batched Huffman: device + pinned staging (hist/first of every string, then the pack tables)
    iec::Buf<uint8_t> d_batch;
    iec::Buf<uint8_t, iec::Mem::Pinned> h_batch;
    // pipelined batches: two pinned slots for the histogram read-back and two for the pack tables,
    // each guarded by an event (no stream-wide synchronisation between batches)
    iec::Buf<uint8_t, iec::Mem::Pinned> h_hist[2];
    iec::Event ev_hist[2];
    int hist_count[2] = {};
    iec::Buf<uint8_t, iec::Mem::Pinned> h_pack[2];
    iec::Event ev_pack[2];         // the table copy out of pinned slot i (on tab_stream)
    bool pack_recorded[2] = {};
    iec::Buf<uint8_t> d_pack[2];   // device table slots
    iec::Event ev_packed[2];       // the pack (and prefix copies) that read device slot i
    bool packed_recorded[2] = {};
    int pack_slot = 0;
    int fused_count = 0;  // > 0: the last encode (ie_encode_images_counted) left this many histograms in d_chist
    // the counted pipeline: the encoder's histograms (cleared by the first-occurrence pass that reads
    // them: chist_zero_rows), and per pinned slot the device n / first / unresolved the rare first_full
    // pass of ie_huffman_hist_batch_wait needs, with the batch it reads
    iec::Buf<uint32_t> d_chist;
    // leading 256-word rows of d_chist known to be zero (the counted encode skips its memset when
    // its rows lie within them), and the rows that will be zero once the fused pass has read -- and
    // cleared -- the last counted encode's rows
    size_t chist_zero_rows = 0, chist_clean_after = 0;
    bool hist_skip_zero = false;  // one shot: encode() skips its histogram memset (set by the counted encode)
    iec::Buf<uint8_t> d_cslot[2];
    bool hist_fused[2] = {};
    const uint8_t* hist_in[2] = {};
    size_t hist_pitch[2] = {};
    // decoder scratch
    iec::Buf<uint8_t> d_dec;           // staged stream + padding
    // 8-byte words.  Record decode: 32-bit arrays carved by dec_scratch (ie_capi_decode.cpp) -- the
    // chunks' record bases and counts, the count workgroups' totals, the top-level entries, the
    // speculative exits.  Huffman decode: [cap] chunk entries, [cap] symbol bases, 130 words of
    // top-level entries.
    iec::Buf<uint64_t> d_walk;
    iec::Buf<uint32_t> d_count;        // Huffman decode: per-chunk symbol counts, then the walk workgroups' totals
    iec::Buf<uint16_t> d_rtab;         // chunk transfer tables and the composites of every level (record and Huffman parse)
    iec::Buf<uint16_t> d_rpos;         // record parse: record positions per chunk
    // [8].  Record decode: [2] the speculative parse's fail flag.  Huffman decode: [1] the changed /
    // invalid flag pair, [2] the symbol total.  ie_huffman_hist: [3] its unresolved-bytes word.
    // ([0] and [4..7] are unused, and [1] by the record decode.)
    iec::Buf<uint64_t> d_misc;
    // record decode results, pinned host memory the device writes directly through h_decres.dev()
    // ([0] end bit, [1] record total): no read-back copy
    iec::Buf<uint64_t, iec::Mem::Mapped> h_decres;
    // ie_decode_images: [count][2] the same pair per image, then [count] the images' stream lengths
    // on their way to d_imgbits (the device writes the pairs through h_imgres.dev())
    iec::Buf<uint64_t, iec::Mem::Mapped> h_imgres;
    iec::Buf<uint64_t> d_imgbits;      // stream bits of every image (device)
    iec::Buf<uint16_t> d_hlut;         // Huffman decode prefix table (32768 entries)
    iec::Buf<uint8_t> d_hout;          // Huffman decode output staging (host destinations)
    // ie_huffman_decode_batch.  d_hufb: the scratch of one sub-batch, per image and sized from the
    // longest stream, one array per kind holding every image's part in turn (HufScratch,
    // ie_capi_huffman.cpp).  d_hufb_res, 8-byte words for the whole batch: [n] stream bits, [n] first
    // code bits, [n] flag pairs (capacity, invalid code), [n] symbol totals; h_hufb_res: its pinned
    // mirror (the first two arrays go up, the last two come back in the call's one read).
    iec::Buf<uint8_t> d_hufb;
    iec::Buf<uint64_t> d_hufb_res;
    iec::Buf<uint8_t, iec::Mem::Pinned> h_hufb_res;
    iec::Buf<uint8_t> d_pix;
    iec::Buf<uint8_t> d_region;        // region and scaled decodes into host memory: rw*rh pixels per frame, packed
    int last_chunks = 0;               // chunks of the last record decode
    int last_groups = 0;               // and their groups
    int last_spec = 0;                 // 1: the last record decode was the speculative parse
    int spec_parse = 0;                // ie_set_exact_parse(ctx, 0): speculative record parse first
    int spec_warm = 0;                 // ie_set_spec_warm(ctx, w): w warm-up chunks (<= 8)
    iec::Buf<unsigned long long> d_first;   // [256]
    ie_pipe* pipe = nullptr;           // streamed host path of image batches (created on first use)
    ie_vdec* vdec = nullptr;           // the open streamed video decoder (one per context; its owner closes it)
    // P-frame videos (ie_encode_gop): reconstructed frames (two, alternating), the prediction
    // error's coefficients and record lengths, the scan's tile sums, the frames' bit positions
    iec::Buf<uint8_t> d_gop_rec;
    iec::Buf<int16_t> d_gop_coef;
    iec::Buf<uint32_t> d_gop_bits;
    iec::Buf<uint64_t> d_gop_tile;
    iec::Buf<uint64_t> d_gop_pos;
    // ie_encode_gop_groups: one wave of groups' scratch, carved per kind (every group's slot, then
    // every group's reconstructed frames, coefficients, record lengths, tile sums; the wave's
    // position table and the groups' first bits).  The frames' positions in the stream: d_gop_pos.
    iec::Buf<uint8_t> d_gopg;
    // The probes (ie_capi_probe.cpp): the candidate matrices (zig-zag order; pinned, then device:
    // IE_PROBE_MAX of them), the event after the copy out of the pinned block, the sums when the
    // results are host memory (with sse: bits, then sse, read back together into h_probe_out)
    iec::Buf<uint16_t, iec::Mem::Pinned> h_probe_q;
    iec::Buf<uint16_t> d_probe_q;
    iec::Event ev_probe;
    bool probe_recorded = false;
    iec::Buf<uint64_t> d_probe_bits;
    iec::Buf<uint64_t, iec::Mem::Pinned> h_probe_out;
    // the gop probes: the frames of every (group, candidate) pair of one wave (ie_probe_gop: two
    // reconstructions; ie_probe_gop_rd: two reconstructions, then two decoded frames)
    iec::Buf<uint8_t> d_probe_gop;
};

namespace iec {

inline int fail(ie_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPCHK(ctx, expr)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return iec::fail(ctx, IE_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
    } while (0)

// hipMemoryTypeDevice / hipMemoryTypeHost (pinned); anything else, pageable memory included, is neither
inline bool is_ptr_type(const void* p, hipMemoryType type) {
    if (!p) return false;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == type;
}
inline bool is_device_ptr(const void* p) { return is_ptr_type(p, hipMemoryTypeDevice); }
inline bool is_pinned_ptr(const void* p) { return is_ptr_type(p, hipMemoryTypeHost); }

template <class T, Mem K>
int Buf<T, K>::reserve(ie_ctx* c, size_t elems, Wait wait) {
    if (p_ && cap_ >= elems) return IE_OK;
    const size_t n = std::max(elems, cap_ + cap_ / 2);
    if (p_) {
        if (wait == Wait::Stream) HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, release());
    }
    void* p = nullptr;
    if (K == Mem::Device)
        HIPCHK(c, hipMalloc(&p, n * sizeof(T)));
    else
        HIPCHK(c, hipHostMalloc(&p, n * sizeof(T),
                                K == Mem::Mapped ? hipHostMallocMapped | hipHostMallocCoherent : hipHostMallocDefault));
    p_ = static_cast<T*>(p);
    if (K == Mem::Mapped) {  // (a failure here leaves cap() at 0: the next reserve starts over)
        HIPCHK(c, hipHostGetDevicePointer(&p, p_, 0));
        dev_ = static_cast<T*>(p);
    }
    cap_ = n;
    return IE_OK;
}

inline int Event::create(ie_ctx* c, unsigned flags) {
    if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, flags));
    return IE_OK;
}
inline int Stream::create(ie_ctx* c, unsigned flags) {
    if (!s) HIPCHK(c, hipStreamCreateWithFlags(&s, flags));
    return IE_OK;
}

// The device's view of plain pinned host memory (any hipHostMalloc under unified addressing).
template <class T>
int device_view(ie_ctx* c, T* host, T** dev) {
    void* dp = nullptr;
    HIPCHK(c, hipHostGetDevicePointer(&dp, host, 0));
    *dev = static_cast<T*>(dp);
    return IE_OK;
}

// ---- ie_tables.cpp: a pure function of (n, q), no device involved
bool build_tables(int n, const uint16_t* q, ie::EncTables* T);

// ---- ie_capi.cpp: launch state, error counters, shared checks and staging
int prepare_state(ie_ctx* c, int ntiles, int nframes);
int stage_mark(ie_ctx* c, int i);
int read_errors(ie_ctx* c, unsigned* timeouts, uint64_t* fallbacks);
void note_async(ie_ctx* c, const char* what);
// A look-back timeout with nothing left to re-run: IE_EDEVICE, the message with `where` appended.
int lookback_failed(ie_ctx* c, const char* where = "");
// After a synchronous launch's error read: no timeouts -> IE_OK, *redo = false.  Otherwise the
// dispatch order did not hold: already ordering tiles by ticket -> IE_EDEVICE; else the context
// switches to ticket mode and *redo = true (the caller cleans up what it must and runs again).
int ticket_redo(ie_ctx* c, unsigned timeouts, bool* redo);
int check_dims(ie_ctx* c, int w, int h, int nframes);
// check_dims, then stride >= w, then (nframes > 1) frame_pitch covers a frame -- in that order
int check_frames(ie_ctx* c, int w, int h, int nframes, size_t stride, size_t frame_pitch);
// Host bytes (frames, or a byte string) go to d_in on the stream; device bytes are used in place.
int stage_in(ie_ctx* c, const uint8_t* src, bool src_dev, size_t bytes, const uint8_t** dsrc);

// bytes from the first pixel of the first frame to the last pixel of the last
inline size_t frames_span(int nframes, size_t frame_pitch, size_t stride, int w, int h) {
    return size_t(nframes - 1) * frame_pitch + stride * size_t(h - 1) + size_t(w);
}
inline size_t bound_bits_per_block(int n) { return 4 + 16 * size_t(n * n + 1); }
// bits_needed of an int16 (utils.hpp:226-243): Frame::MVEC_BIT_SIZE = bits_needed(merange) (VideoBase.cpp:42)
inline int mvec_bits(int merange) {
    int b = 1;
    const int16_t v = int16_t(merange);
    while (int16_t(int16_t((v & ((1 << b) - 1)) << (16 - b)) >> (16 - b)) != v) b++;
    return b;
}

struct Geometry {
    int bx, by, gpr, gpf, tpf, ntiles;
};
inline Geometry geometry(int w, int h, int n, int nframes) {
    Geometry g;
    const int bpt = ie::encode_blocks_per_thread(n);
    g.bx = w / n;
    g.by = h / n;
    g.gpr = (g.bx + bpt - 1) / bpt;
    g.gpf = g.gpr * g.by;
    const int tpt = ie::encode_threads_per_tile();  // groups per tile
    g.tpf = (g.gpf + tpt - 1) / tpt;
    g.ntiles = g.tpf * nframes;
    return g;
}

// ---- ie_capi_encode.cpp
// One encode launch over device-resident frames (no staging, no synchronisation): the EncArgs
// of ie_device.h, the chain state's epoch and the launch.  start_dev (optional) makes the chain
// start at a device-resident bit position (the previous launch's chain end, ie_vstream_*);
// chain_end (optional) receives the chain end(s) instead of the context's d_chain_end.
struct Launch {
    const uint8_t* dy = nullptr;
    int w = 0, h = 0;
    size_t stride = 0, frame_pitch = 0;
    int nframes = 0, use_rle = 1, mode = IE_MODE_FAST;
    uint32_t* dout = nullptr;  // word 0 = stream bytes [0, 4) (may point before the allocation)
    size_t out_pitch = 0;      // segmented: bytes between images
    uint64_t start_bit = 0;
    const uint64_t* start_dev = nullptr;
    uint64_t* chain_end = nullptr;
    int segmented = 0;
    int16_t* coef = nullptr;
    uint32_t* hist = nullptr;
    Launch(const uint8_t* dy_, int w_, int h_, size_t stride_, size_t frame_pitch_, int nframes_, int use_rle_, int mode_,
           uint32_t* dout_, uint64_t start_bit_)
        : dy(dy_), w(w_), h(h_), stride(stride_), frame_pitch(frame_pitch_), nframes(nframes_), use_rle(use_rle_),
          mode(mode_), dout(dout_), start_bit(start_bit_) {}
};
int launch_chain(ie_ctx* c, const Launch& L);
// Common driver of ie_encode_frames (segmented = 0) and ie_encode_images (segmented = 1).
int encode(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
           int use_rle, int mode, uint8_t* out, size_t out_cap, size_t out_pitch, uint64_t start_bit,
           int segmented, uint64_t* frame_bits, uint64_t* end_bits, int16_t* coef = nullptr,
           uint32_t* hist = nullptr);
// What every P-frame entry point checks before any device work (gop already >= 1); *need:
// ie_gop_stream_bound of the call, IE_ECAP when out_cap is below it.
int check_gop(ie_ctx* c, int w, int h, size_t stride, size_t frame_pitch, int nframes, int gop, int merange,
              size_t out_cap, uint64_t start_bit, size_t* need);
// One wave of groups of pictures encoded side by side (ie_encode_gop_groups; a chunk of a gop > 1
// ie_vstream): the context's group scratch (d_gopg) carved for up to Gw groups.
struct GopWave {
    int gop = 0;
    size_t Gw = 0;  // groups the scratch holds
    size_t sz_slot = 0, sz_rec = 0, sz_coef = 0, sz_bits = 0, sz_tile = 0;  // bytes per group
    uint32_t* slots = nullptr;
    uint8_t* rec = nullptr;
    int16_t* coef = nullptr;
    uint32_t* bits = nullptr;
    uint64_t *tile = nullptr, *pos = nullptr, *goff = nullptr;
};
// Groups per wave: `want`, at most 65535 (grid.y), at most what keeps the scratch under 1 GiB, at
// most IE_GOP_BATCH_MAX (read on every call), at least 1.
size_t gop_wave_groups(int n, int w, int h, int gop, int merange, size_t want);
// Grows d_gopg if it must and carves it.  The pointers hold until another call grows it: carve
// again before every run of launches.
int gop_wave_scratch(ie_ctx* c, int w, int h, int gop, int merange, size_t Gw, GopWave* W);
// The launches of one wave over device frames wy (gw <= W.Gw groups, nfw frames, only the last
// group may be short), no synchronisation: zero the slots, the I-frames as a batch of independent
// images, steps 1 .. gop-1 of the P-frames, the splice into dout from *base_dev (null: start_bit).
// fpos[0 .. nfw] receives the frames' first bits in dout and the wave's end bit.
int launch_gop_wave(ie_ctx* c, const GopWave& W, const uint8_t* wy, int w, int h, size_t stride, size_t frame_pitch,
                    int gw, int nfw, int merange, int use_rle, int mode, uint32_t* dout, uint64_t start_bit,
                    const uint64_t* base_dev, uint64_t* fpos);

// ---- ie_capi_decode.cpp: the record parse's chunk plan and scratch (ie_capi_vdec.cpp plans its
// chunks of frames with them)
constexpr uint64_t kMaxChunkBits = uint64_t(1) << 15;  // (16-bit record positions)
// Chunk plan of a record span (span bits from the first record, nblocks records).
struct RecPlan {
    uint64_t C;       // chunk bits
    int nchunks;
    size_t tab_rows;  // rows of D entries: the chunks' tables and every level's composites
    int levels;
};
// n: the block size of the stream (the context's, or the one a streamed decoder took at open)
int plan_chunks(ie_ctx* c, int n, uint64_t span, uint64_t nblocks, uint64_t cmax, RecPlan* plan);
int dec_scratch(ie_ctx* c, int n, const RecPlan& pl, size_t batch, ie::RecParseArgs& a, uint32_t** spec = nullptr);
// ... and what ie_capi_region.cpp shares with the full decoders: the staging of the record stream
// (a 16-byte aligned device stream is read in place unless `always`), the pixel destination (a
// device `out` itself, else buf grown to span bytes), the decode arguments, and the batch call's
// length checks, sub-batch size and stream staging (ie_decode_images)
int stage_stream_in(ie_ctx* c, Buf<uint8_t>& buf, const uint8_t* in, size_t len, bool always, const uint8_t** words);
int pixel_dest(ie_ctx* c, Buf<uint8_t>& buf, uint8_t* out, size_t span, bool* out_dev, uint8_t** dpix);
ie::DecArgs dec_args(const ie_ctx* c, int w, int h, int use_rle, size_t stride);
int check_image_bits(ie_ctx* c, size_t in_pitch, const uint64_t* nbits, int count, uint64_t start_bit, uint64_t* max_bits);
size_t dec_batch_images(int n, const RecPlan& pl, int count);
int stage_image_streams(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                        uint64_t max_bits, const uint8_t** words, size_t* pitch);

// ---- ie_capi_region.cpp: decodes that write part of every frame (region and scaled decode)
// The decode pass such a call launches after the parse: (parse arguments, decode arguments with the
// destination set, block size, images, batch, stream) -> composition levels, < 0 on failure.
using PartLaunch = std::function<int(const ie::RecParseArgs&, const ie::DecArgs&, int, int, bool, hipStream_t)>;
// The body of a call that decodes rw x rh pixels per frame of a stream of w x h frames, behind its
// checks of the dimensions and the destination: the start_bit check of ie_decode_frames, stream
// staging, chunk plan, `launch`, one synchronisation, IE_EFORMAT as the full decode, and for a host
// `out` the packed buffer d_region and the copy of its rows of rw bytes.
int decode_part(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes, int use_rle, int rw,
                int rh, uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit, const PartLaunch& launch);
// The same for a batch of images (ie_decode_images' nbits checks, sub-batches and per-image errors).
int decode_images_part(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count, uint64_t start_bit,
                       int w, int h, int use_rle, int rw, int rh, uint8_t* out, size_t stride, size_t frame_pitch,
                       uint64_t* end_bits, const PartLaunch& launch);

// ---- ie_capi_stream.cpp: host frames in, host streams out
// IE_CHUNK_MB's pixel target of a streamed chunk (default 8 MiB; ie_vstream and ie_vdec)
size_t chunk_target();
int streamed_images(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                    int use_rle, int mode, uint8_t* out, size_t out_pitch, uint64_t start_bit, uint64_t* end_bits);
int streamed_frames(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                    int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit, uint64_t* frame_bits,
                    uint64_t* end_bit);
void pipe_free(ie_pipe* p);

}  // namespace iec
