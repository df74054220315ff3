// imageencoder_amd/csrc/ie_capi_decode.cpp -- the record decoders of the C ABI: the chunk plan and
// scratch layout of the record parse, the staging of streams and pixel destinations, and
// ie_decode_frames / ie_decode_images / ie_decode_gop.
#include "ie_ctx.hpp"

#if IE_PROFILE
#include <chrono>
#endif

using namespace iec;

// The record stream on the device for the kernels' reads: whole aligned words up to the one holding
// the last byte, then zeros (16 bytes of padding for the vector loads).  A 16-byte aligned device
// stream is read in place unless `always`; anything else is copied (device copy or H2D) into buf.
int iec::stage_stream_in(ie_ctx* c, Buf<uint8_t>& buf, const uint8_t* in, size_t len, bool always, const uint8_t** words) {
    const bool in_dev = is_device_ptr(in);
    *words = in;
    if (!always && in_dev && !(reinterpret_cast<uintptr_t>(in) & 15u)) return IE_OK;
    const size_t padded = (len + 3) / 4 * 4 + 16;
    int r = buf.reserve(c, padded);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(buf + (len / 4) * 4, 0, padded - (len / 4) * 4, c->stream));
    HIPCHK(c, hipMemcpyAsync(buf, in, len, in_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    *words = buf;
    return IE_OK;
}

// Where the kernels write pixels: a device destination itself, or buf (grown to span bytes) for a
// host one -- which copy_frames_out then fills, pixel rows only (the bytes between rows and frames
// belong to the caller).
int iec::pixel_dest(ie_ctx* c, Buf<uint8_t>& buf, uint8_t* out, size_t span, bool* out_dev, uint8_t** dpix) {
    *out_dev = is_device_ptr(out);
    *dpix = out;
    if (*out_dev) return IE_OK;
    int r = buf.reserve(c, span);
    *dpix = buf;
    return r;
}
namespace {
int copy_frames_out(ie_ctx* c, uint8_t* out, const uint8_t* dpix, int f0, int f1, int w, int h, size_t stride,
                    size_t frame_pitch) {
    for (int f = f0; f < f1; f++)
        HIPCHK(c, hipMemcpy2D(out + size_t(f) * frame_pitch, stride, dpix + size_t(f) * frame_pitch, stride, size_t(w),
                              size_t(h), hipMemcpyDeviceToHost));
    return IE_OK;
}
}  // namespace

// The decode arguments every path shares; nframes, out, frame_pitch and add_base are the caller's.
ie::DecArgs iec::dec_args(const ie_ctx* c, int w, int h, int use_rle, size_t stride) {
    ie::DecArgs da{};
    da.bx = w / c->n;
    da.by = h / c->n;
    da.rle = use_rle ? 1 : 0;
    da.stride = stride;
    da.tab = c->d_tab;
    return da;
}

namespace {
#ifndef IE_GOP_CAPC
#define IE_GOP_CAPC 1  // 0: (A/B builds) gop decode chunks sized by the I-frame bound alone
#endif

}  // namespace

// Chunk plan of a record span (RecPlan, ie_ctx.hpp) for block size n.
int iec::plan_chunks(ie_ctx* c, int n, uint64_t span, uint64_t nblocks, uint64_t cmax, RecPlan* plan) {
    // chunking: about R records per chunk (IE_DEC_R; default 24 for 4x4, 28 for 8x8: measured
    // with 32-table composition groups on 4K noise / mixed / gradient / flat frames and the
    // reference's ex1 / ex4 -- 4x4 against 16, 24, 32, 48: ex4 126 -> 115 us, mixed 197 -> 191 us,
    // noise and flat unchanged; 8x8 against 20-32: noise 342 -> 258 us, ex1 376 -> 269 us,
    // gradient 209 -> 181 us, flat 101 -> 112 us; 8x8 noise alone is erratic in R, 2.6x slower at
    // 24) so that every chunk's walks are short; C a multiple of 32, at least
    // 256 bits, at most 2^15 (16-bit record positions; a table wave's LDS -- the chunk's bits and
    // valid-header bitmap -- stays small)
    static const char* rs = getenv("IE_DEC_R");
    const uint64_t recs = rs ? std::max<uint64_t>(1, strtoull(rs, nullptr, 10)) : (n == 4 ? 24 : 28);
    const uint64_t want = std::max<uint64_t>((nblocks + recs - 1) / recs, 1);
    uint64_t C = (span + want - 1) / want;
    C = std::min<uint64_t>(std::max<uint64_t>((C + 31) / 32 * 32, 256), std::max<uint64_t>(cmax / 32 * 32, 256));
    const uint64_t nch = std::max<uint64_t>((span + C - 1) / C, 1);
    // levels: ceil(n / G) composites per level until at most G remain (kRecMaxLevels levels at
    // most), counted by the code that launches them
    int levels = 0;
    const size_t tab_rows = ie::rec_table_rows(size_t(nch), n, &levels);
    if (levels > ie::kRecMaxLevels || nch > uint64_t(INT32_MAX))
        return fail(c, IE_EINVAL, "stream too long for one decode call");
    *plan = {C, int(nch), tab_rows, levels};
    return IE_OK;
}

// Scratch of one image under a plan, and of `batch` images side by side.  Per image: its tables and
// composites (img_tab entries, a multiple of 8 so that every image's start 16-byte aligned) and
// kRecPosCap positions per chunk; in d_walk, as 32-bit words, one array per kind holding every
// image's part in turn -- record bases and counts [nchunks], count workgroups' totals [nwg],
// top-level entries [G] -- then the speculative exits [nchunks] (single stream only).  Every
// array starts on an 8-byte word.
namespace {
struct DecScratch {
    size_t img_tab, nwg, img_bytes;
    int seg;
};
DecScratch dec_scratch_size(int n, const RecPlan& pl) {
    DecScratch s;
    const size_t nch = size_t(pl.nchunks), G = size_t(ie::rec_group_chunks(n));
    s.seg = ie::rec_count_seg(uint32_t(pl.C));
    s.nwg = (nch + 4 * size_t(s.seg) - 1) / (4 * size_t(s.seg));
    s.img_tab = (pl.tab_rows * size_t(ie::rec_entry_span(n)) + 7) / 8 * 8;
    s.img_bytes = s.img_tab * 2 + nch * ie::kRecPosCap * 2 + (2 * nch + s.nwg + G) * 4;
    return s;
}
}  // namespace
// Grows the parse buffers for `batch` images and fills a's chunking fields, scratch pointers and
// batch strides (the single-stream kernels ignore the strides).  The record stream's own fields
// (words, nbits, start_bit, dstart, total, end_out) are the caller's.  *spec (optional): the exits.
int iec::dec_scratch(ie_ctx* c, int n, const RecPlan& pl, size_t batch, ie::RecParseArgs& a, uint32_t** spec) {
    const DecScratch s = dec_scratch_size(n, pl);
    const size_t nch = size_t(pl.nchunks), G = size_t(ie::rec_group_chunks(n));
    auto even = [](size_t words32) { return (words32 + 1) / 2 * 2; };
    const size_t cnt_at = even(batch * nch), wg_at = cnt_at + even(batch * nch), e_at = wg_at + even(batch * s.nwg);
    const size_t spec_at = e_at + even(batch * G), end = spec_at + (spec ? even(nch) : 0);
    int r;
    if ((r = c->d_rtab.reserve(c, batch * s.img_tab))) return r;
    if ((r = c->d_rpos.reserve(c, batch * nch * ie::kRecPosCap))) return r;
    if ((r = c->d_walk.reserve(c, end / 2 + 1))) return r;
    uint32_t* u32 = reinterpret_cast<uint32_t*>(c->d_walk.get());
    a.C = uint32_t(pl.C);
    a.nchunks = pl.nchunks;
    a.seg = s.seg;
    a.tab = c->d_rtab;
    a.pos = c->d_rpos;
    a.lbase = u32;
    a.cnt = u32 + cnt_at;
    a.wgsum = u32 + wg_at;
    a.E = u32 + e_at;
    if (spec) *spec = u32 + spec_at;
    a.img_tab = s.img_tab;
    a.img_chunks = uint32_t(nch);
    a.img_wg = uint32_t(s.nwg);
    a.img_E = uint32_t(G);
    return IE_OK;
}

// ie_decode_images' checks of the streams' lengths; *max_bits: the longest.
int iec::check_image_bits(ie_ctx* c, size_t in_pitch, const uint64_t* nbits, int count, uint64_t start_bit,
                          uint64_t* max_bits) {
    *max_bits = 0;
    for (int k = 0; k < count; k++) {
        if (nbits[k] / 8 > in_pitch || nbits[k] > uint64_t(in_pitch) * 8)
            return fail(c, IE_EINVAL, "image " + std::to_string(k) + ": nbits beyond its slot of in_pitch bytes");
        if (start_bit > nbits[k]) return fail(c, IE_EINVAL, "image " + std::to_string(k) + ": start_bit beyond the stream");
        *max_bits = std::max(*max_bits, nbits[k]);
    }
    return IE_OK;
}

// Images per sub-batch: what keeps the scratch within 1 GiB, at most IE_DEC_BATCH_MAX, at most count.
size_t iec::dec_batch_images(int n, const RecPlan& pl, int count) {
    size_t batch = std::max<size_t>(1, (size_t(1) << 30) / dec_scratch_size(n, pl).img_bytes);
    if (const char* eb = getenv("IE_DEC_BATCH_MAX"))  // (read on every call: a limit in images, only ever lower)
        if (atoi(eb) > 0) batch = std::min<size_t>(batch, size_t(atoi(eb)));
    return std::min<size_t>(batch, size_t(count));
}

// The batch's stream lengths to d_imgbits and its streams where the kernels read them (*words,
// slots *pitch bytes apart); h_imgres is grown for the result pairs.
int iec::stage_image_streams(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                             uint64_t max_bits, const uint8_t** words_out, size_t* pitch_out) {
    int r;
    if ((r = c->d_imgbits.reserve(c, size_t(count)))) return r;
    if ((r = c->h_imgres.reserve(c, 3 * std::max<size_t>(size_t(count), 16)))) return r;
    // the stream lengths: through pinned memory into a device array (every workgroup reads its
    // image's; a read of host memory per workgroup would cost more than the copy)
    uint64_t* h_bits = c->h_imgres + 2 * size_t(count);
    std::memcpy(h_bits, nbits, size_t(count) * sizeof(uint64_t));
    HIPCHK(c, hipMemcpyAsync(c->d_imgbits, h_bits, size_t(count) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    // streams: device slots that are 16-byte aligned, 16-byte pitched are read in place (16-byte
    // vector loads of whole aligned groups inside [0, nbits[k]), single words up to the one holding
    // the last bit -- inside the slot, as in_pitch is a multiple of 4 -- and the bits at or past
    // nbits[k] are cleared by the kernels); anything else is staged into such slots, zero padded
    const bool in_dev = is_device_ptr(in);
    const uint8_t* words = in;
    size_t pitch = in_pitch;
    if (!in_dev || (reinterpret_cast<uintptr_t>(in) & 15u) || (in_pitch & 15u)) {
        const size_t max_bytes = size_t((max_bits + 7) / 8);
        pitch = (max_bytes + 15) / 16 * 16 + 16;
        if ((r = c->d_dec.reserve(c, pitch * size_t(count)))) return r;
        HIPCHK(c, hipMemsetAsync(c->d_dec, 0, pitch * size_t(count), c->stream));
        if (in_dev) {
            HIPCHK(c, hipMemcpy2DAsync(c->d_dec, pitch, in, in_pitch, std::min(max_bytes, in_pitch), size_t(count),
                                       hipMemcpyDeviceToDevice, c->stream));
        } else {
            for (int k = 0; k < count; k++)
                if (nbits[k])
                    HIPCHK(c, hipMemcpyAsync(c->d_dec + size_t(k) * pitch, in + size_t(k) * in_pitch,
                                             size_t((nbits[k] + 7) / 8), hipMemcpyHostToDevice, c->stream));
        }
        words = c->d_dec;
    }
    *words_out = words;
    *pitch_out = pitch;
    return IE_OK;
}

namespace {

// Profiling of the single-stream record decode (IE_PROFILE builds, tools/prof_decode.py and
// tools/dec_stamps.py): host-side phase times and the table pass's per-wave stamps (IE_DEC_STAMPS =
// file: [table waves][8] u64 per call).  Empty in the product.
#if IE_PROFILE
struct DecHostTimes {
    double pre = 0, launch = 0, sync = 0;
    long n = 0;
    ~DecHostTimes() {
        if (n) fprintf(stderr, "[dec host] %ld calls: before the first launch %.1f us, launches %.1f us, sync %.1f us\n", n,
                       pre / n, launch / n, sync / n);
    }
};
DecHostTimes g_dht;
struct DecProfile {
    static double now() {
        return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }
    double t0 = now(), t1 = 0, t2 = 0;
    const char* stamps = getenv("IE_DEC_STAMPS");
    Buf<uint64_t> d_ws;
    size_t nws = 0;
    int begin(ie_ctx* c, ie::RecParseArgs& pa) {  // before the first launch
        int tm = 1, hb = 0;
        ie::rec_table_geometry(pa.C, c->n, &tm, &hb);
        nws = size_t(pa.nchunks + tm - 1) / size_t(tm) * 8;
        if (stamps) {
            if (int r = d_ws.reserve(c, nws)) return r;
            HIPCHK(c, hipMemsetAsync(d_ws, 0, nws * 8, c->stream));
            pa.wstamp = reinterpret_cast<unsigned long long*>(d_ws.get());
        }
        t1 = now();
        return IE_OK;
    }
    void launched() { t2 = now(); }  // after the speculative attempt, before the exact parse
    int end(ie_ctx* c, const ie::RecParseArgs&) {  // after the synchronisation
        g_dht.pre += t1 - t0;
        g_dht.launch += t2 - t1;
        g_dht.sync += now() - t2;
        g_dht.n++;
        if (d_ws) {
            std::vector<uint64_t> hws(nws);
            HIPCHK(c, hipMemcpy(hws.data(), d_ws, nws * 8, hipMemcpyDeviceToHost));
            if (FILE* f = fopen(stamps, "ab")) {
                fwrite(hws.data(), 8, nws, f);
                fclose(f);
            }
        }
        return IE_OK;
    }
};
#else
struct DecProfile {
    int begin(ie_ctx*, ie::RecParseArgs&) { return IE_OK; }
    void launched() {}
    int end(ie_ctx*, const ie::RecParseArgs&) { return IE_OK; }
};
#endif

}  // namespace

extern "C" {

int ie_decode_frames(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes,
                     int use_rle, uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit) {
    if (!c || !in || !out) return IE_EINVAL;
    DecProfile prof;
    int r = check_frames(c, w, h, nframes, stride, frame_pitch);
    if (r) return r;
    if (start_bit > uint64_t(len) * 8) return fail(c, IE_EINVAL, "start_bit beyond the stream");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->n;
    // (the kernels read the stream with 16-byte vector loads of whole aligned words up to the one
    // holding the last byte -- never past its page -- and clear the bits past the stream themselves)
    const uint8_t* words;
    if ((r = stage_stream_in(c, c->d_dec, in, len, false, &words))) return r;
    const uint64_t nbits = uint64_t(len) * 8;
    const uint64_t nblocks = uint64_t(nframes) * (w / n) * (h / n);
    RecPlan pl{};
    ie::RecParseArgs pa{};
    uint32_t* spec_exits = nullptr;
    if ((r = plan_chunks(c, n, nbits - start_bit, nblocks, kMaxChunkBits, &pl))) return r;
    if ((r = dec_scratch(c, n, pl, 1, pa, &spec_exits))) return r;
    int levels = pl.levels;
    bool out_dev;
    uint8_t* dpix;
    if ((r = pixel_dest(c, c->d_pix, out, frames_span(nframes, frame_pitch, stride, w, h), &out_dev, &dpix)))
        return r;
    ie::DecArgs da = dec_args(c, w, h, use_rle, stride);
    da.nframes = nframes;
    da.out = dpix;
    da.frame_pitch = frame_pitch;
    pa.words = reinterpret_cast<const uint32_t*>(words);
    pa.nbits = nbits;
    pa.start_bit = start_bit;
    pa.rle = da.rle;
    if ((r = c->h_decres.reserve(c, 8))) return r;
    pa.total = c->h_decres.dev() + 1;
    pa.end_out = c->h_decres.dev();
    // (the result words need no clearing: the last chunk's decode wave always writes the record total,
    // and the end bit is read only when that total covers the last block, whose decode writes it)
    if ((r = prof.begin(c, pa))) return r;
    // Optional speculative parse first (ie_decode.hip rec_spec_kernel; ie_set_exact_parse(ctx, 0)
    // or IE_DEC_SPEC=1): each chunk's entry is where a walk from an earlier chunk's first bit left
    // it, verified by the count pass; on any mismatch (e.g. periodic content, whose wrong-phase
    // walks never meet the true path) nothing was decoded and the exact parse over composed
    // transfer tables runs.  Off by default: measured on 4K frames and the reference's example
    // images it wins only on flat content -- a wrong-phase walk takes ~35 steps to
    // meet the true path and the slowest of ~16 000 chunks sets the pass's time.
    static const char* es = getenv("IE_DEC_SPEC");
    const bool spec = (es && atoi(es) != 0) || c->spec_parse;
    bool exact = !spec;
    c->last_spec = 0;
    if (spec) {
        pa.spec = spec_exits;
        pa.fail = reinterpret_cast<unsigned*>(c->d_misc + 2);
        // warm-up chunks: a speculative walk crosses this many whole chunks (about 32 (4x4) / 16
        // (8x8) records each) before the chunk whose exit it reports (IE_DEC_WARM)
        static const char* ew = getenv("IE_DEC_WARM");
        const int warm = c->spec_warm ? c->spec_warm : (ew ? std::max(0, std::min(8, atoi(ew))) : 0);
        // rec_spec_kernel stages seg + warm chunks per wave in LDS: keep a wave within 12 KB
        const int room = int((uint64_t(12 * 1024) * 8 - 256) / uint64_t(pa.C)) - pa.seg;
        pa.warm = std::max(0, std::min(warm, room));
        ie::launch_rec_spec_decode(pa, da, n, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->h_decres[1] == ~0ull) {
            exact = true;
            pa.spec = nullptr;
            pa.fail = nullptr;
        } else {
            c->last_spec = 1;
            levels = 0;
        }
    }
    prof.launched();
    if (exact) {
        if (ie::launch_rec_parse_decode(pa, da, n, c->stream) < 0) return fail(c, IE_EINVAL, "stream too long for one decode call");
        HIPCHK(c, hipGetLastError());
    }
    c->last_chunks = pa.nchunks;
    c->last_groups = levels;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((r = prof.end(c, pa))) return r;
    const uint64_t end = c->h_decres[0], total = c->h_decres[1];
    if (total < nblocks || end > nbits) return fail(c, IE_EFORMAT, "stream ends before the last block");
    if (!out_dev && (r = copy_frames_out(c, out, dpix, 0, nframes, w, h, stride, frame_pitch))) return r;
    if (end_bit) *end_bit = end;
    return IE_OK;
}

// A batch of independent images through ONE set of launches: every pass of the exact record parse
// gains the image as its grid's y dimension (ie_decode.hip, the kernels' batch instantiations), so
// the launch chain, the synchronisation and the result read are paid once.  One chunk plan for the
// batch: C from the longest stream, nchunks its chunk count; a shorter stream's trailing chunks
// hold no record.  Scratch is per image (tables + composites, position lists, walk arrays); a batch
// whose scratch would pass 1 GiB (dec_batch_images) runs as sub-batches, one after another on the stream,
// and the call still waits once.
int ie_decode_images(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count, uint64_t start_bit,
                     int w, int h, int use_rle, uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bits) {
    if (!c || !in || !nbits || !out) return IE_EINVAL;
    int r = check_frames(c, w, h, count, stride, frame_pitch);
    if (r) return r;
    uint64_t max_bits = 0;
    if ((r = check_image_bits(c, in_pitch, nbits, count, start_bit, &max_bits))) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->n;
    const uint64_t nblocks = uint64_t(w / n) * (h / n);
    RecPlan pl{};
    if ((r = plan_chunks(c, n, max_bits - start_bit, nblocks, kMaxChunkBits, &pl))) return r;
    const size_t batch = dec_batch_images(n, pl, count);
    ie::RecParseArgs pa{};
    if ((r = dec_scratch(c, n, pl, batch, pa))) return r;
    const uint8_t* words;
    size_t pitch;
    if ((r = stage_image_streams(c, in, in_pitch, nbits, count, max_bits, &words, &pitch))) return r;
    bool out_dev;
    uint8_t* dpix;
    if ((r = pixel_dest(c, c->d_pix, out, frames_span(count, frame_pitch, stride, w, h), &out_dev, &dpix)))
        return r;
    ie::DecArgs da = dec_args(c, w, h, use_rle, stride);
    da.nframes = 1;
    da.frame_pitch = frame_pitch;
    pa.start_bit = start_bit;
    pa.rle = da.rle;
    pa.img_words = pitch / 4;
    int levels = 0;
    for (size_t k0 = 0; k0 < size_t(count); k0 += batch) {  // (sub-batches share the scratch: stream order)
        const int m = int(std::min(batch, size_t(count) - k0));
        pa.words = reinterpret_cast<const uint32_t*>(words + k0 * pitch);
        pa.img_nbits = c->d_imgbits + k0;
        pa.end_out = c->h_imgres.dev() + 2 * k0;
        pa.total = c->h_imgres.dev() + 2 * k0 + 1;
        da.out = dpix + k0 * frame_pitch;
        levels = ie::launch_rec_parse_decode_images(pa, da, n, m, c->stream);
        if (levels < 0) return fail(c, IE_EINVAL, "stream too long for one decode call");
        HIPCHK(c, hipGetLastError());
    }
    c->last_chunks = pl.nchunks;
    c->last_groups = levels;
    c->last_spec = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // (every image's last chunk wrote its record total; its end bit is read only when that total
    // covers the last block, whose decode wrote it)
    int bad = -1;
    for (int k = count - 1; k >= 0; k--) {
        const uint64_t end = c->h_imgres[2 * k], total = c->h_imgres[2 * k + 1];
        const bool ok = total >= nblocks && end <= nbits[k];
        if (!ok) bad = k;
        if (end_bits) end_bits[k] = ok ? end : UINT64_MAX;
        if (ok && !out_dev && (r = copy_frames_out(c, out, dpix, k, k + 1, w, h, stride, frame_pitch))) return r;
    }
    if (bad >= 0) return fail(c, IE_EFORMAT, "image " + std::to_string(bad) + ": stream ends before the last block");
    return IE_OK;
}

// Video decode with P-frames (VideoDecoder.cpp:28-58, Frame.cpp:47-127): frame by frame, each
// starting at the previous frame's end; a P-frame's motion vectors and reference-block copies
// (pf_mvcopy_kernel), then its records (every microblock's) decoded onto the copied pixels.
// Device-chained: every frame's launches read its first bit from the device word the previous
// frame's decode wrote (pos[f], RecParseArgs::dstart), with chunks planned from the frame's bound
// rather than its span, so the whole call is enqueued at once and the host waits once, at the end,
// for the end bits and record totals it checks.
int ie_decode_gop(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes, int gop,
                  int merange, int use_rle, int motioncomp, uint8_t* out, size_t stride, size_t frame_pitch,
                  uint64_t* end_bit) {
    if (!c || !in || !out) return IE_EINVAL;
    int r = check_dims(c, w, h, nframes);  // (reported before a bad merange; check_frames passes it again)
    if (r) return r;
    gop = std::max(1, gop);
    if (merange < 0 || merange > 32767) return fail(c, IE_EINVAL, "merange must be in [0, 32767]");
    if ((r = check_frames(c, w, h, nframes, stride, frame_pitch))) return r;
    if (gop > 1 && nframes > 1 && (w % 16 || h % 16))
        return fail(c, IE_EINVAL, "P-frames decode for W and H multiples of 16 only: the reference's macroblocks are "
                                  "misplaced otherwise and its uncovered microblocks read records never written");
    if (start_bit > uint64_t(len) * 8) return fail(c, IE_EINVAL, "start_bit beyond the stream");
    HIPCHK(c, hipSetDevice(c->device));
    // the stream once on the device (16-byte aligned, zero padding for the vector reads), the
    // frames decoded into a device buffer (P-frames read their predecessor there)
    const uint8_t* words;
    if ((r = stage_stream_in(c, c->d_in, in, len, true, &words))) return r;
    bool out_dev;
    uint8_t* dpix;
    if ((r = pixel_dest(c, c->d_gop_rec, out, frames_span(nframes, frame_pitch, stride, w, h), &out_dev,
                        &dpix)))
        return r;
    const int n = c->n, mv = mvec_bits(merange);
    const uint64_t nbits = uint64_t(len) * 8;
    const uint64_t nmb = uint64_t(w / 16) * (h / 16), mvb = nmb * 2u * uint64_t(mv);
    const uint64_t nblocks = uint64_t(w / n) * (h / n);
    const uint64_t rec_bound = nblocks * bound_bits_per_block(n);
    // per-frame device words: pos[0..nframes] first bits (pos[f + 1] = frame f's end), tot[f]
    // records on frame f's true path; then the host copy of both
    const size_t nw = 2 * size_t(nframes) + 1;
    if ((r = c->d_gop_pos.reserve(c, nw))) return r;
    uint64_t* pos = c->d_gop_pos;
    uint64_t* tot = pos + nframes + 1;
    ie::launch_gop_init(pos, tot, nframes, start_bit, c->stream);
    HIPCHK(c, hipGetLastError());
    // one chunk plan for every frame: its bound (plus a P-frame's vectors), so the grids and
    // scratch do not depend on where a frame ends
    RecPlan pl{};
    ie::RecParseArgs pa{};
    // (gop > 1: the plan is sized by the I-frame bound, but a P-frame's records are a few bits each
    // -- at most kRecPosCap records per chunk keeps its chunks on the listed-positions decode
    // instead of the re-walk.  With RLE the shortest record is bl = 0: its 4 header bits alone.
    // Without RLE the bound is the shortest record an encoder writes, bl = 1 (the 4-bit bl = 0
    // record is valid there too; chunks dense with them take the re-walk))
    const uint64_t min_rec = use_rle ? 4u : uint64_t(4 + n * n);
    const uint64_t cmax = (gop > 1 && IE_GOP_CAPC) ? uint64_t(ie::kRecPosCap) * min_rec : kMaxChunkBits;
    if ((r = plan_chunks(c, n, rec_bound, nblocks, cmax, &pl))) return r;
    if ((r = dec_scratch(c, n, pl, 1, pa))) return r;
    ie::DecArgs da = dec_args(c, w, h, use_rle, stride);
    da.nframes = 1;
    pa.words = reinterpret_cast<const uint32_t*>(words);
    pa.nbits = nbits;
    pa.rle = da.rle;
    pa.span = rec_bound;
    if (gop > 1 && nframes > 1 && !motioncomp)
        if ((r = c->d_gop_coef.reserve(c, (stride * size_t(h) + 1) / 2))) return r;
    for (int f = 0; f < nframes; f++) {
        uint8_t* fo = dpix + size_t(f) * frame_pitch;
        const bool iframe = (f % gop) == 0;
        if (!iframe) {
            ie::launch_pframe_mvcopy(words, 0, pos + f, nbits, mv, fo - frame_pitch, stride, fo, stride, w, h, c->stream);
            HIPCHK(c, hipGetLastError());
        }
        // add_base: the decoded prediction error is added to the pixels already there.  Without
        // motion compensation the error is read (the stream must be consumed) but not applied:
        // decoded into scratch
        const bool apply = iframe || motioncomp;
        da.out = apply ? fo : reinterpret_cast<uint8_t*>(c->d_gop_coef.get());
        da.add_base = (apply && !iframe) ? 1 : 0;
        pa.dstart = pos + f;
        pa.start_add = iframe ? 0 : mvb;
        pa.total = tot + f;
        pa.end_out = pos + f + 1;
        if (ie::launch_rec_parse_decode(pa, da, n, c->stream) < 0) return fail(c, IE_EINVAL, "stream too long for one decode call");
        HIPCHK(c, hipGetLastError());
    }
    std::vector<uint64_t> hp(nw);
    HIPCHK(c, hipMemcpyAsync(hp.data(), pos, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last_chunks = pa.nchunks;
    c->last_groups = pl.levels;
    c->last_spec = 0;
    for (int f = 0; f < nframes; f++) {
        if ((f % gop) != 0 && hp[f] + mvb > nbits) return fail(c, IE_EFORMAT, "stream ends in the motion vectors");
        if (hp[nframes + 1 + f] < nblocks || hp[f + 1] > nbits) return fail(c, IE_EFORMAT, "stream ends before the last block");
    }
    if (!out_dev && (r = copy_frames_out(c, out, dpix, 0, nframes, w, h, stride, frame_pitch))) return r;
    if (end_bit) *end_bit = hp[nframes];
    return IE_OK;
}

int ie_last_decode_info(ie_ctx* c, int* chunks, int* levels) {
    if (!c) return IE_EINVAL;
    if (chunks) *chunks = c->last_chunks;
    if (levels) *levels = c->last_groups;
    return IE_OK;
}

int ie_set_exact_parse(ie_ctx* c, int exact) {
    if (!c) return IE_EINVAL;
    c->spec_parse = exact != 0 ? 0 : 1;  // any nonzero value: the exact parse
    return IE_OK;
}

int ie_set_spec_warm(ie_ctx* c, int warm) {
    if (!c) return IE_EINVAL;
    c->spec_warm = warm < 0 ? 0 : (warm > 8 ? 8 : warm);  // clamped before use: no negation
    return IE_OK;
}

int ie_last_decode_spec(ie_ctx* c) { return c ? c->last_spec : 0; }

}  // extern "C"
