// imageencoder_amd/csrc/ie_capi_encode.cpp -- the encode drivers of the C ABI: the launch of one
// tile chain, the staged ie_encode_frames / ie_encode_images path, quantise-only, P-frame videos
// frame by frame (ie_encode_gop) and with their groups of pictures side by side (ie_encode_gop_groups).
#include "ie_ctx.hpp"

using namespace iec;

namespace iec {

int launch_chain(ie_ctx* c, const Launch& L) {
    const int bpt = ie::encode_blocks_per_thread(c->n);
    const Geometry g = geometry(L.w, L.h, c->n, L.nframes);
    // a launch too small to fill the chip: its tiles reach the look-back together (deep windows)
    const bool small = g.ntiles < ie::encode_small_tiles();
    // every row piece starts on a multiple of m bytes: the base, the stride and (several frames) the pitch do
    auto rows_aligned = [&L](size_t m) {
        return reinterpret_cast<uintptr_t>(L.dy) % m == 0 && L.stride % m == 0 &&
               (L.nframes == 1 || L.frame_pitch % m == 0);
    };
    const bool vec_ok = rows_aligned(size_t(bpt * c->n));  // a group's row: 16 bytes (4x4), 8 bytes (8x8)
    const bool vec16 = rows_aligned(16);  // a 16-byte load or DMA of a row piece is naturally aligned
    int r;
    ie::EncArgs a{};
    a.y = L.dy;
    a.stride = L.stride;
    a.frame_pitch = L.frame_pitch;
    a.w = L.w;
    a.h = L.h;
    a.nframes = L.nframes;
    a.bx = g.bx;
    a.by = g.by;
    a.gpr = g.gpr;
    a.gpr_magic = (g.gpr > 1) ? uint32_t(((uint64_t(1) << 32) + uint64_t(g.gpr) - 1) / uint64_t(g.gpr)) : 0u;
    a.groups_per_frame = g.gpf;
    a.tiles_per_frame = g.tpf;
    a.div_frames = ie::make_fastdiv(uint32_t(L.nframes));
    a.div_tpf = ie::make_fastdiv(uint32_t(g.tpf));
    a.div_gpr = ie::make_fastdiv(uint32_t(g.gpr));
    a.ntiles = g.ntiles;
    a.rle = L.use_rle ? 1 : 0;
    a.segmented = L.segmented;
    a.vec_ok = (vec_ok ? ie::kVecGroup : 0) | (vec16 ? ie::kVec16 : 0);
    a.out = L.dout;
    a.out_pitch_words = L.segmented ? L.out_pitch / 4 : 0;
    a.start_bit = L.start_bit;
    a.start_dev = L.start_dev;
    a.tab = c->d_tab;
    a.rec_bits = c->h_tab->rec_bits;
    a.tri = (c->n == 4 && (a.rec_bits - 4) / 17 <= 10) ? 1 : 0;  // bl_max = (rec_bits - 4) / (1 + N*N); 3 bl <= 30
    a.coef = L.coef;
    a.hist = L.hist;
#if IE_PROFILE  // (profiling builds only: ie_ctx.hpp)
    static const int ablate = getenv("IE_ABLATE") ? atoi(getenv("IE_ABLATE")) : 0;
    static const char* stamp_file = getenv("IE_STAMPS");  // per-tile phase stamps
#else
    constexpr int ablate = 0;
    const char* stamp_file = nullptr;
#endif
    a.ablate = ablate | IE_ABLATE_FORCE;  // IE_ABLATE_FORCE: A/B builds of an ablation
    if ((r = prepare_state(c, g.ntiles, L.nframes))) return r;
    a.st = c->d_state;
    a.ticket = c->use_ticket ? c->d_ticket : nullptr;
    a.ticket_base = c->ticket_base;
    a.tag = c->tag;
    a.frame_start = c->d_frame_start;
    a.chain_end = L.chain_end ? L.chain_end : c->d_chain_end;
    a.err = c->d_err;
    a.wave_fix = c->d_wave_fix;
    c->last_fix_words = 0;  // (set after the launch: its kernel's waves per tile)
    if (L.hist && !c->hist_skip_zero) HIPCHK(c, hipMemsetAsync(L.hist, 0, size_t(L.nframes) * 256 * sizeof(uint32_t), c->stream));
    c->hist_skip_zero = false;  // (a re-launch clears)
    uint64_t* d_stamps = nullptr;
    if (stamp_file) {
        HIPCHK(c, hipMalloc(&d_stamps, size_t(g.ntiles) * ie::kStamps * sizeof(uint64_t)));
        HIPCHK(c, hipMemsetAsync(d_stamps, 0, size_t(g.ntiles) * ie::kStamps * sizeof(uint64_t), c->stream));
    }
    a.stamps = d_stamps;
    a.deep_lb = small ? 1 : 0;
    const int fix_per_tile = ie::launch_encode(a, c->n, L.mode == IE_MODE_EXACT, c->stream);
    c->last_fix_words = (L.mode == IE_MODE_EXACT) ? 0 : g.ntiles * fix_per_tile;
    HIPCHK(c, hipGetLastError());
    if (d_stamps) {
        std::vector<uint64_t> hs(size_t(g.ntiles) * ie::kStamps);
        HIPCHK(c, hipMemcpyAsync(hs.data(), d_stamps, hs.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(d_stamps));
        if (FILE* f = std::fopen(stamp_file, "wb")) {
            std::fwrite(hs.data(), sizeof(uint64_t), hs.size(), f);
            std::fclose(f);
        }
    }
    if (c->use_ticket) c->ticket_base += uint64_t(g.ntiles);
    return IE_OK;
}

int encode(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
           int use_rle, int mode, uint8_t* out, size_t out_cap, size_t out_pitch, uint64_t start_bit,
           int segmented, uint64_t* frame_bits, uint64_t* end_bits, int16_t* coef, uint32_t* hist) {
    c->fused_count = 0;  // any encode replaces the batch scratch's meaning
    int r = check_frames(c, w, h, nframes, stride, frame_pitch);
    if (r) return r;
    if (segmented && (out_pitch % 4)) return fail(c, IE_EINVAL, "out_pitch must be a multiple of 4");
    HIPCHK(c, hipSetDevice(c->device));
    const Geometry g = geometry(w, h, c->n, nframes);
    const int nchains = segmented ? nframes : 1;

    // output bound
    const uint64_t payload_bound = uint64_t(g.bx) * g.by * bound_bits_per_block(c->n) * (segmented ? 1 : nframes);
    const uint64_t end_bound = start_bit + payload_bound;
    const size_t need_bytes = size_t((end_bound + 31) / 32) * 4;
    const size_t span = segmented ? out_pitch * size_t(nframes - 1) + need_bytes : need_bytes;
    if (segmented && out_pitch < need_bytes) return fail(c, IE_ECAP, "out_pitch below ie_stream_bound");
    if (out_cap < span) return fail(c, IE_ECAP, "output capacity below ie_stream_bound");
    const bool in_dev = is_device_ptr(y), out_dev = is_device_ptr(out);

    // Host frames in AND host streams out, several frames: the streamed path (pinned double
    // buffering, H2D / encode / D2H on three streams; ie_vstream for the concatenated chain).
    if (!in_dev && !out_dev && nframes > 1 && !coef && !hist && !c->use_ticket) {
        return segmented ? streamed_images(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_pitch,
                                           start_bit, end_bits)
                         : streamed_frames(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_cap,
                                           start_bit, frame_bits, end_bits);
    }

    // input
    const uint8_t* dy;
    if ((r = stage_in(c, y, in_dev, frames_span(nframes, frame_pitch, stride, w, h), &dy))) return r;

    // output
    uint32_t* dout;
    const uint64_t w0 = start_bit / 32;
    if (out_dev) {
        if (reinterpret_cast<uintptr_t>(out) % 4) return fail(c, IE_EINVAL, "device output must be 4-byte aligned");
        dout = reinterpret_cast<uint32_t*>(out);
    } else {
        // stage from the word holding start_bit; its leading bytes carry the caller's header
        const size_t stage = span - size_t(w0) * 4;
        if ((r = c->d_out.reserve(c, stage))) return r;
        for (int f = 0; f < (segmented ? nframes : 1); f++) {
            const size_t hb = size_t(f) * out_pitch + size_t(w0) * 4;
            uint8_t word[4] = {0, 0, 0, 0};
            for (int e = 0; e < 4 && hb + e < out_cap; e++) word[e] = out[hb + e];
            // keep only the bytes before start_bit's byte plus its leading bits
            HIPCHK(c, hipMemcpyAsync(c->d_out + size_t(f) * out_pitch, word, 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        dout = reinterpret_cast<uint32_t*>(c->d_out.get()) - w0;
    }

    Launch L(dy, w, h, stride, frame_pitch, nframes, use_rle, mode, dout, start_bit);
    L.out_pitch = out_pitch;
    L.segmented = segmented;
    L.coef = coef;
    L.hist = hist;
    if ((r = launch_chain(c, L))) return r;

    if (!frame_bits && !end_bits && out_dev) {  // nothing to read back
        note_async(c, hist ? "counting encode" : "encode");
        return IE_OK;
    }
    std::vector<uint64_t> fs(nframes), ce(nchains);
    HIPCHK(c, hipMemcpyAsync(fs.data(), c->d_frame_start, nframes * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ce.data(), c->d_chain_end, nchains * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    unsigned timeouts = 0;
    if ((r = read_errors(c, &timeouts, &c->last_fallbacks))) return r;
    bool redo;
    if ((r = ticket_redo(c, timeouts, &redo))) return r;
    if (redo)
        return encode(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_cap, out_pitch, start_bit,
                      segmented, frame_bits, end_bits, coef, hist);
    if (!out_dev) {
        for (int ch = 0; ch < nchains; ch++) {
            const size_t b0 = size_t(ch) * out_pitch + size_t(start_bit / 8);
            const size_t b1 = size_t(ch) * out_pitch + size_t((ce[ch] + 7) / 8);
            const size_t off = b0 - (size_t(ch) * out_pitch + size_t(w0) * 4);
            HIPCHK(c, hipMemcpy(out + b0, c->d_out + size_t(ch) * out_pitch + off, b1 - b0, hipMemcpyDeviceToHost));
        }
    }
    if (frame_bits)  // a frame ends where the next one starts, or at its chain's end
        for (int f = 0; f < nframes; f++)
            frame_bits[f] = (segmented ? ce[f] : (f + 1 < nframes) ? fs[f + 1] : ce[0]) - fs[f];
    if (end_bits) std::copy(ce.begin(), ce.end(), end_bits);
    return IE_OK;
}

}  // namespace iec

extern "C" {

size_t ie_stream_bound(int w, int h, int n, int nframes, uint64_t start_bit) {
    if ((n != 4 && n != 8) || w <= 0 || h <= 0 || nframes <= 0) return 0;
    const uint64_t bits = start_bit + uint64_t(w / n) * (h / n) * bound_bits_per_block(n) * nframes;
    return size_t((bits + 31) / 32) * 4;
}

int ie_encode_frames(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                     int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit, uint64_t* frame_bits,
                     uint64_t* end_bit) {
    if (!c || !y || !out) return IE_EINVAL;
    return encode(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_cap, 0, start_bit, 0,
                  frame_bits, end_bit);
}

size_t ie_gop_stream_bound(int w, int h, int n, int nframes, int merange, uint64_t start_bit) {
    if ((n != 4 && n != 8) || w <= 0 || h <= 0 || nframes <= 0 || merange < 0 || merange > 32767) return 0;
    const uint64_t per_frame = uint64_t(w / n) * (h / n) * bound_bits_per_block(n) +
                               uint64_t(w / 16) * (h / 16) * 2u * uint64_t(mvec_bits(merange));
    return size_t((start_bit + per_frame * uint64_t(nframes) + 31) / 32) * 4 + 8;
}

}  // extern "C"

namespace iec {

// What ie_encode_gop, ie_encode_gop_groups and ie_vstream_open_gop check before any device work, in
// this order; gop is already >= 1.  *need: ie_gop_stream_bound of the call.
int check_gop(ie_ctx* c, int w, int h, size_t stride, size_t frame_pitch, int nframes, int gop, int merange,
              size_t out_cap, uint64_t start_bit, size_t* need) {
    int r = check_dims(c, w, h, nframes);  // (reported before a bad merange; check_frames passes it again)
    if (r) return r;
    if (merange < 0 || merange > 32767) return fail(c, IE_EINVAL, "merange must be in [0, 32767] (15-bit header field)");
    if ((r = check_frames(c, w, h, nframes, stride, frame_pitch))) return r;
    const bool has_p = gop > 1 && nframes > 1;
    if (has_p && w % 16 && h / 16 >= 2)
        return fail(c, IE_EINVAL, "P-frames need W % 16 == 0 when H >= 32: the reference builds its macroblocks "
                                  "from misplaced, overlapping rows there (ImageBase.cpp:223-227)");
    *need = ie_gop_stream_bound(w, h, c->n, nframes, merange, start_bit);
    if (out_cap < *need) return fail(c, IE_ECAP, "output capacity below ie_gop_stream_bound");
    return IE_OK;
}

static size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// Scratch per group: the slot, two reconstructed frames, the prediction error's coefficients
// (4x4 only) and record lengths, the tile sums, and its column of the position table.
static void gop_wave_sizes(int n, int w, int h, int gop, int merange, GopWave* W) {
    const int nb = (w / n) * (h / n);
    W->gop = gop;
    W->sz_slot = align256(ie_gop_stream_bound(w, h, n, gop, merange, 0));
    W->sz_rec = align256(2 * size_t(w) * h);
    W->sz_coef = n == 4 ? align256(size_t(nb) * 16 * sizeof(int16_t)) : 0;
    W->sz_bits = align256(size_t(nb) * sizeof(uint32_t));
    W->sz_tile = align256((size_t(ie::pframe_tiles(nb)) + 1) * sizeof(uint64_t));
}

size_t gop_wave_groups(int n, int w, int h, int gop, int merange, size_t want) {
    GopWave W;
    gop_wave_sizes(n, w, h, gop, merange, &W);
    const size_t per_group = W.sz_slot + W.sz_rec + W.sz_coef + W.sz_bits + W.sz_tile + (size_t(gop) + 2) * sizeof(uint64_t);
    size_t Gw = std::min<size_t>({std::max<size_t>(want, 1), 65535, std::max<size_t>(1, ((size_t(1) << 30) - 1024) / per_group)});
    if (const char* eb = getenv("IE_GOP_BATCH_MAX"))  // (read on every call: a limit in groups, only ever lower)
        if (atoll(eb) > 0) Gw = std::min<size_t>(Gw, size_t(atoll(eb)));
    return Gw;
}

int gop_wave_scratch(ie_ctx* c, int w, int h, int gop, int merange, size_t Gw, GopWave* W) {
    gop_wave_sizes(c->n, w, h, gop, merange, W);
    W->Gw = Gw;
    const size_t sz_pos = align256((size_t(gop) + 1) * Gw * sizeof(uint64_t));
    const size_t sz_goff = align256((Gw + 1) * sizeof(uint64_t));
    int r = c->d_gopg.reserve(c, Gw * (W->sz_slot + W->sz_rec + W->sz_coef + W->sz_bits + W->sz_tile) + sz_pos + sz_goff);
    if (r) return r;
    uint8_t* p = c->d_gopg;
    auto carve = [&p](size_t bytes) {
        uint8_t* q = p;
        p += bytes;
        return q;
    };
    W->slots = reinterpret_cast<uint32_t*>(carve(Gw * W->sz_slot));
    W->rec = carve(Gw * W->sz_rec);
    W->coef = reinterpret_cast<int16_t*>(carve(Gw * W->sz_coef));
    W->bits = reinterpret_cast<uint32_t*>(carve(Gw * W->sz_bits));
    W->tile = reinterpret_cast<uint64_t*>(carve(Gw * W->sz_tile));
    W->pos = reinterpret_cast<uint64_t*>(carve(sz_pos));  // [gop + 1][groups of the wave]
    W->goff = reinterpret_cast<uint64_t*>(carve(sz_goff));
    return IE_OK;
}

int launch_gop_wave(ie_ctx* c, const GopWave& W, const uint8_t* wy, int w, int h, size_t stride, size_t frame_pitch,
                    int gw, int nfw, int merange, int use_rle, int mode, uint32_t* dout, uint64_t start_bit,
                    const uint64_t* base_dev, uint64_t* fpos) {
    const int n = c->n, gop = W.gop, bx = w / n;
    const size_t fpx = size_t(w) * h, group_pitch = size_t(gop) * frame_pitch;
    int r;
    HIPCHK(c, hipMemsetAsync(W.slots, 0, size_t(gw) * W.sz_slot, c->stream));
    HIPCHK(c, hipMemsetAsync(W.pos, 0, size_t(gw) * sizeof(uint64_t), c->stream));  // every slot starts at bit 0
    {  // step 0: the I-frames, a batch of independent images; their end bits are pos[1][g]
        Launch L(wy, w, h, stride, group_pitch, gw, use_rle, mode, W.slots, 0);
        L.segmented = 1;
        L.out_pitch = W.sz_slot;
        L.chain_end = W.pos + gw;
        if ((r = launch_chain(c, L))) return r;
    }
    for (int j = 1; j < gop && j < nfw; j++) {  // step j: frame j of the groups that have one
        ie::PfArgs a{};
        a.cur = wy + size_t(j) * frame_pitch;
        a.cs = stride;
        a.g_cur = group_pitch;
        if (j == 1) {  // the I-frame as the caller holds it
            a.ref = wy;
            a.rs = stride;
            a.g_ref = group_pitch;
        } else {       // the previous P-frame's reconstruction
            a.ref = W.rec + size_t((j - 1) & 1) * fpx;
            a.rs = size_t(w);
            a.g_ref = W.sz_rec;
        }
        a.rec = W.rec + size_t(j & 1) * fpx;
        a.g_rec = W.sz_rec;
        a.w = w;
        a.h = h;
        a.mbx = w / 16;
        a.mby = h / 16;
        a.bx = bx;
        a.rle = use_rle ? 1 : 0;
        a.merange = merange;
        a.mv_bits = mvec_bits(merange);
        a.tab = c->d_tab;
        a.coef = W.coef;
        a.g_coef = W.sz_coef / sizeof(int16_t);
        a.bits = W.bits;
        a.g_bits = W.sz_bits / sizeof(uint32_t);
        a.g_tile = W.sz_tile / sizeof(uint64_t);
        a.out = W.slots;
        a.g_out = W.sz_slot / sizeof(uint32_t);
        a.start = W.pos + size_t(j) * gw;
        a.end = W.pos + size_t(j + 1) * gw;
        const int gj = std::min(gw, (nfw - j + gop - 1) / gop);
        ie::launch_pframe_groups(a, n, gj, W.tile, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    ie::GopSplice sp{};
    sp.pos = W.pos;
    sp.groups = gw;
    sp.gop = gop;
    sp.nframes = nfw;
    sp.slots = W.slots;
    sp.slot_words = W.sz_slot / sizeof(uint32_t);
    sp.out = dout;
    sp.base = start_bit;
    sp.base_dev = base_dev;
    sp.goff = W.goff;
    sp.fpos = fpos;
    ie::launch_gop_splice(sp, c->stream);
    HIPCHK(c, hipGetLastError());
    return IE_OK;
}

}  // namespace iec

namespace {

// Where the P-frame payload is built: the caller's device stream, or zeroed staging (the P-frame
// records are ORed in) holding the caller's leading bytes.  Word 0 of *dout = stream bytes [0, 4).
int stage_gop_out(ie_ctx* c, uint8_t* out, bool out_dev, size_t need, uint64_t start_bit, uint32_t** dout) {
    if (out_dev) {
        if (reinterpret_cast<uintptr_t>(out) % 4) return fail(c, IE_EINVAL, "device output must be 4-byte aligned");
        *dout = reinterpret_cast<uint32_t*>(out);
        return IE_OK;
    }
    int r = c->d_out.reserve(c, need);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(c->d_out, 0, need, c->stream));
    const size_t hb = size_t((start_bit + 7) / 8);
    if (hb) HIPCHK(c, hipMemcpyAsync(c->d_out, out, hb, hipMemcpyHostToDevice, c->stream));
    *dout = reinterpret_cast<uint32_t*>(c->d_out.get());
    return IE_OK;
}

// Before a P-frame video is redone in ticket mode on a device-resident stream: the first attempt
// ORed vectors and P-frame records at positions derived from a bad end bit, so the caller's
// stream is cleared from start_bit on (the bits before it are the caller's).
int clear_gop_stream(ie_ctx* c, uint8_t* out, uint64_t start_bit, size_t need) {
    const size_t b0 = size_t(start_bit / 8), b1 = size_t((start_bit + 7) / 8);
    auto lead_bits = [&](bool set) {  // start_bit's byte (b1 > b0): its bits from start_bit on, set or cleared
        uint8_t lead = 0;
        HIPCHK(c, hipMemcpyAsync(&lead, out + b0, 1, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        lead = set ? lead | uint8_t(0xFFu >> (start_bit % 8)) : lead & uint8_t(0xFF00u >> (start_bit % 8));
        HIPCHK(c, hipMemcpyAsync(out + b0, &lead, 1, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return int(IE_OK);
    };
    int r;
    if (c->fake_fired) {  // debug: a faked timeout stands for a bad first attempt -- leave junk
        c->fake_fired = false;
        HIPCHK(c, hipMemsetAsync(out + b0 + (b1 > b0 ? 1 : 0), 0xA5, need - b1, c->stream));
        if (b1 > b0 && (r = lead_bits(true))) return r;
    }
    if (need > b1) HIPCHK(c, hipMemsetAsync(out + b1, 0, need - b1, c->stream));
    if (b1 > b0 && (r = lead_bits(false))) return r;
    return IE_OK;
}

}  // namespace

extern "C" {

// The frame loop of VideoEncoder.cpp:83-91 with I- and P-frames (VideoBase.cpp:96-122): I-frames
// through the block encoder, P-frames through ie_pframe.hip; every frame starts at the previous
// frame's end bit read on the device, and a P-frame's reference is the previous frame's buffer as
// the reference leaves it (an I-frame's own pixels, a P-frame's reconstruction).
int ie_encode_gop(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes, int gop,
                  int merange, int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit,
                  uint64_t* frame_bits, uint64_t* end_bit) {
    if (!c || !y || !out) return IE_EINVAL;
    gop = std::max(1, gop);
    size_t need = 0;
    int r = check_gop(c, w, h, stride, frame_pitch, nframes, gop, merange, out_cap, start_bit, &need);
    if (r) return r;
    const bool has_p = gop > 1 && nframes > 1;
    HIPCHK(c, hipSetDevice(c->device));
    const bool in_dev = is_device_ptr(y), out_dev = is_device_ptr(out);

    const uint8_t* dy;
    if ((r = stage_in(c, y, in_dev, frames_span(nframes, frame_pitch, stride, w, h), &dy))) return r;
    uint32_t* dout;
    if ((r = stage_gop_out(c, out, out_dev, need, start_bit, &dout))) return r;
    const int n = c->n, bx = w / n, nb = bx * (h / n);
    if (has_p) {
        if ((r = c->d_gop_rec.reserve(c, 2 * size_t(w) * h))) return r;
        if ((r = c->d_gop_coef.reserve(c, size_t(nb) * 16))) return r;
        if ((r = c->d_gop_bits.reserve(c, size_t(nb)))) return r;
        if ((r = c->d_gop_tile.reserve(c, size_t(ie::pframe_tiles(nb)) + 1))) return r;
    }
    if ((r = c->d_gop_pos.reserve(c, size_t(nframes) + 1))) return r;
    HIPCHK(c, hipMemcpy(c->d_gop_pos, &start_bit, sizeof(uint64_t), hipMemcpyHostToDevice));

    const uint8_t* ref = nullptr;
    size_t rs = 0;
    for (int f = 0; f < nframes; f++) {
        const uint8_t* cf = dy + size_t(f) * frame_pitch;
        if (f % gop == 0) {
            Launch L(cf, w, h, stride, 0, 1, use_rle, mode, dout, start_bit);
            L.start_dev = c->d_gop_pos + f;
            L.chain_end = c->d_gop_pos + f + 1;
            if ((r = launch_chain(c, L))) return r;
            ref = cf;
            rs = stride;
        } else {
            ie::PfArgs a{};
            a.cur = cf;
            a.cs = stride;
            a.ref = ref;
            a.rs = rs;
            a.rec = c->d_gop_rec + size_t(f & 1) * size_t(w) * h;
            a.w = w;
            a.h = h;
            a.mbx = w / 16;
            a.mby = h / 16;
            a.bx = bx;
            a.rle = use_rle ? 1 : 0;
            a.merange = merange;
            a.mv_bits = mvec_bits(merange);
            a.tab = c->d_tab;
            a.coef = c->d_gop_coef;
            a.bits = c->d_gop_bits;
            a.out = dout;
            a.start = c->d_gop_pos + f;
            a.end = c->d_gop_pos + f + 1;
            if (n == 4 && !c->use_ticket) {  // the record tiles' scan by look-back (one launch)
                if ((r = prepare_state(c, ie::pframe_tiles(nb), 1))) return r;
                a.st = c->d_state;
                a.tag = c->tag;
                a.err = c->d_err;
            }
            ie::launch_pframe(a, n, c->d_gop_tile, c->stream);
            HIPCHK(c, hipGetLastError());
            ref = a.rec;
            rs = size_t(w);
        }
    }
    std::vector<uint64_t> pos(size_t(nframes) + 1);
    HIPCHK(c, hipMemcpyAsync(pos.data(), c->d_gop_pos, pos.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    unsigned timeouts = 0;
    if ((r = read_errors(c, &timeouts, nullptr))) return r;
    bool redo;
    if ((r = ticket_redo(c, timeouts, &redo))) return r;
    if (redo) {  // an I-frame's tiles did not run in order: redo in ticket mode
        if (out_dev && (r = clear_gop_stream(c, out, start_bit, need))) return r;
        return ie_encode_gop(c, y, w, h, stride, frame_pitch, nframes, gop, merange, use_rle, mode, out, out_cap,
                             start_bit, frame_bits, end_bit);
    }
    if (!out_dev) {
        const size_t b0 = size_t(start_bit / 8), b1 = size_t((pos[nframes] + 7) / 8);
        HIPCHK(c, hipMemcpy(out + b0, c->d_out + b0, b1 - b0, hipMemcpyDeviceToHost));
    }
    if (frame_bits)
        for (int f = 0; f < nframes; f++) frame_bits[f] = pos[f + 1] - pos[f];
    if (end_bit) *end_bit = pos[nframes];
    return IE_OK;
}

// ie_encode_gop with the groups of pictures side by side.  An I-frame resets the prediction, so a
// group takes nothing from its predecessors but the bit its payload starts at: every group is
// encoded into a zeroed slot of its own from bit 0 -- step 0 the I-frames as one batch of
// independent images (the launch of ie_encode_images), step j the j-th frame of every group that
// has one (launch_pframe_groups: always a prefix of the groups) -- and gop_splice_kernel moves the
// slots' payloads end to end into the stream.  The launch sequence is as deep as gop, not nframes.
int ie_encode_gop_groups(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                         int gop, int merange, int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit,
                         uint64_t* frame_bits, uint64_t* end_bit) {
    if (!c || !y || !out) return IE_EINVAL;
    if (gop <= 1 || nframes <= gop)  // no P-frame, or one group: nothing to run side by side
        return ie_encode_gop(c, y, w, h, stride, frame_pitch, nframes, gop, merange, use_rle, mode, out, out_cap,
                             start_bit, frame_bits, end_bit);
    size_t need = 0;
    int r = check_gop(c, w, h, stride, frame_pitch, nframes, gop, merange, out_cap, start_bit, &need);
    if (r) return r;
    HIPCHK(c, hipSetDevice(c->device));
    const bool in_dev = is_device_ptr(y), out_dev = is_device_ptr(out);
    const uint8_t* dy;
    if ((r = stage_in(c, y, in_dev, frames_span(nframes, frame_pitch, stride, w, h), &dy))) return r;
    uint32_t* dout;
    if ((r = stage_gop_out(c, out, out_dev, need, start_bit, &dout))) return r;

    // A video whose groups' scratch would pass 1 GiB (or 65535 groups: grid.y) runs as waves of
    // groups that share the scratch in stream order (gop_wave_groups; IE_GOP_BATCH_MAX lowers their
    // size further); every wave's splice starts at the previous wave's end bit, read on the device.
    const int G = (nframes + gop - 1) / gop;
    GopWave W;
    if ((r = gop_wave_scratch(c, w, h, gop, merange, gop_wave_groups(c->n, w, h, gop, merange, size_t(G)), &W))) return r;
    if ((r = c->d_gop_pos.reserve(c, size_t(nframes) + 1))) return r;
    for (int g0 = 0; g0 < G; g0 += int(W.Gw)) {
        const int gw = std::min(int(W.Gw), G - g0);
        const int f0 = g0 * gop;  // (< nframes)
        const int nfw = int(std::min<int64_t>(int64_t(nframes) - f0, int64_t(gw) * gop));
        if ((r = launch_gop_wave(c, W, dy + size_t(f0) * frame_pitch, w, h, stride, frame_pitch, gw, nfw, merange, use_rle,
                                 mode, dout, start_bit, g0 ? c->d_gop_pos + f0 : nullptr, c->d_gop_pos + f0)))
            return r;
    }
    std::vector<uint64_t> fp(size_t(nframes) + 1);
    HIPCHK(c, hipMemcpyAsync(fp.data(), c->d_gop_pos, fp.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    unsigned timeouts = 0;
    if ((r = read_errors(c, &timeouts, nullptr))) return r;  // the call's one synchronisation
    bool redo;
    if ((r = ticket_redo(c, timeouts, &redo))) return r;
    if (redo) {  // an I-frame batch's tiles did not run in order: redo in ticket mode
        if (out_dev && (r = clear_gop_stream(c, out, start_bit, need))) return r;
        return ie_encode_gop_groups(c, y, w, h, stride, frame_pitch, nframes, gop, merange, use_rle, mode, out, out_cap,
                                    start_bit, frame_bits, end_bit);
    }
    if (!out_dev) {
        const size_t b0 = size_t(start_bit / 8), b1 = size_t((fp[nframes] + 7) / 8);
        HIPCHK(c, hipMemcpy(out + b0, c->d_out + b0, b1 - b0, hipMemcpyDeviceToHost));
    }
    if (frame_bits)
        for (int f = 0; f < nframes; f++) frame_bits[f] = fp[f + 1] - fp[f];
    if (end_bit) *end_bit = fp[nframes];
    return IE_OK;
}

int ie_encode_images(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                     int use_rle, int mode, uint8_t* out, size_t out_pitch, uint64_t start_bit, uint64_t* end_bits) {
    if (!c || !y || !out) return IE_EINVAL;
    return encode(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_pitch * size_t(nframes),
                  out_pitch, start_bit, 1, nullptr, end_bits);
}

int ie_encode_images_counted(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                             int use_rle, int mode, uint8_t* out, size_t out_pitch, uint64_t start_bit) {
    if (!c || !y || !out || nframes <= 0) return IE_EINVAL;
    // no fused variant (EXACT mode, 8x8 -- its registers are full --, host output): the histogram
    // pass counts later
    if (mode == IE_MODE_EXACT || c->n != 4 || !is_device_ptr(out))
        return ie_encode_images(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_pitch, start_bit,
                                nullptr);
    // the counts go to d_chist, where ie_huffman_hist_batch_ends_async reads (and clears) them: the
    // memset before the launch only when they are not known to be zero
    const size_t K = size_t(nframes);
    int r;
    if (c->d_chist.cap() < K * 256 || !c->d_chist) {
        if ((r = c->d_chist.reserve(c, K * 256))) return r;
        HIPCHK(c, hipMemsetAsync(c->d_chist, 0, c->d_chist.cap() * sizeof(uint32_t), c->stream));
        c->chist_zero_rows = c->d_chist.cap() / 256;
    }
    // rows [0, K) are counted into: skip their memset only when all of them are known zero (rows
    // of an earlier, larger batch that no fused pass cleared may hold stale counts)
    c->hist_skip_zero = K <= c->chist_zero_rows;
    c->chist_clean_after = c->hist_skip_zero ? c->chist_zero_rows : K;
    c->chist_zero_rows = 0;  // dirty until the fused pass reads this batch
    r = encode(c, y, w, h, stride, frame_pitch, nframes, use_rle, mode, out, out_pitch * K, out_pitch, start_bit, 1,
               nullptr, nullptr, nullptr, c->d_chist);
    c->hist_skip_zero = false;
    if (r == IE_OK) c->fused_count = nframes;
    return r;
}

int ie_quantize_frames(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                       int mode, int16_t* coef) {
    if (!c || !y || !coef) return IE_EINVAL;
    int r = check_dims(c, w, h, nframes);
    if (r) return r;
    const size_t bound = ie_stream_bound(w, h, c->n, nframes, 0);
    if ((r = c->d_scratch.reserve(c, bound))) return r;
    const size_t ncoef = size_t(nframes) * (w / c->n) * (h / c->n) * c->n * c->n;
    const bool dev = is_device_ptr(coef);
    int16_t* dc = coef;
    if (!dev) {
        if ((r = c->d_coef.reserve(c, ncoef))) return r;
        dc = c->d_coef;
    }
    uint64_t end = 0;
    r = encode(c, y, w, h, stride, frame_pitch, nframes, 1, mode, c->d_scratch, bound, 0, 0, 0, nullptr, &end, dc);
    if (r) return r;
    if (!dev) HIPCHK(c, hipMemcpy(coef, dc, ncoef * sizeof(int16_t), hipMemcpyDeviceToHost));
    return IE_OK;
}

int ie_last_fallbacks(ie_ctx* c, uint64_t* count) {
    if (!c || !count) return IE_EINVAL;
    unsigned timeouts = 0;
    int r = read_errors(c, &timeouts, &c->last_fallbacks);  // the last encode launch's requests
    if (r) return r;
    *count = c->last_fallbacks;
    if (timeouts) return lookback_failed(c);
    return IE_OK;
}

const uint64_t* ie_last_end_bits(ie_ctx* c) { return c ? c->d_chain_end : nullptr; }

}  // extern "C"
