// imageencoder_amd/csrc/ie_capi_huffman.cpp -- the Huffman pass of the C ABI: histograms (single,
// batched, pipelined), the variable-length pack, the dictionary reader and the decode; ie_bitcopy.
#include "ie_ctx.hpp"

using namespace iec;

namespace {

// Variable-length re-encode of n bytes (Huffman.cpp:314-319) into one stream from start_bit.
int pack(ie_ctx* c, const uint8_t* bytes, size_t n, const uint32_t* code, const uint8_t* len, uint8_t* out,
         size_t out_cap, uint64_t start_bit, uint64_t* end_bit) {
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    unsigned maxlen = 0;
    for (int b = 0; b < 256; b++) {
        if (len[b] > 32) return fail(c, IE_EINVAL, "code length above 32 bits");
        maxlen = std::max<unsigned>(maxlen, len[b]);
    }
    const uint64_t end_bound = start_bit + uint64_t(maxlen) * n;
    const size_t need_bytes = size_t((end_bound + 31) / 32) * 4;
    if (out_cap < need_bytes) return fail(c, IE_ECAP, "output capacity below start_bit + max_len * n bits");
    // code table through pinned memory (the caller's arrays may be gone when the copy runs)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(c->h_code, code, 256 * sizeof(uint32_t));
    std::memcpy(reinterpret_cast<uint8_t*>(c->h_code + 256), len, 256);
    HIPCHK(c, hipMemcpyAsync(c->d_code, c->h_code, 2 * 256 * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    const uint8_t* din;
    if ((r = stage_in(c, bytes, !n || is_device_ptr(bytes), n, &din))) return r;
    const bool out_dev = is_device_ptr(out);
    const uint64_t w0 = start_bit / 32;
    uint32_t* dout;
    if (out_dev) {
        if (reinterpret_cast<uintptr_t>(out) % 4) return fail(c, IE_EINVAL, "device output must be 4-byte aligned");
        dout = reinterpret_cast<uint32_t*>(out);
    } else {
        // (at least the staged word: codes of no bits from a word boundary need no output at all)
        if ((r = c->d_out.reserve(c, std::max<size_t>(need_bytes - size_t(w0) * 4, 4)))) return r;
        uint8_t word[4] = {0, 0, 0, 0};
        for (int e = 0; e < 4 && size_t(w0) * 4 + e < out_cap; e++) word[e] = out[size_t(w0) * 4 + e];
        HIPCHK(c, hipMemcpyAsync(c->d_out, word, 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dout = reinterpret_cast<uint32_t*>(c->d_out.get()) - w0;
    }
    uint64_t end = start_bit;
    if (n) {
        const uint64_t tb = uint64_t(ie::pack_tile_bytes(int(maxlen)));
        const int ntiles = int((n + tb - 1) / tb);
        if ((r = prepare_state(c, ntiles, 1))) return r;
        ie::PackArgs a{};
        a.in = din;
        a.n = n;
        a.code = c->d_code;
        a.len = reinterpret_cast<const uint8_t*>(c->d_code + 256);
        a.ntiles = ntiles;
        a.out = dout;
        a.start_bit = start_bit;
        a.st = c->d_state;
        a.ticket = c->use_ticket ? c->d_ticket : nullptr;
        a.ticket_base = c->ticket_base;
        a.tag = c->tag;
        a.chain_end = c->d_chain_end;
        a.err = c->d_err;
        a.maxlen = int(maxlen);
        ie::launch_pack(a, c->stream);  // (no stage events: ie_last_stage_ms reports the batched calls)
        HIPCHK(c, hipGetLastError());
        if (c->use_ticket) c->ticket_base += uint64_t(ntiles);
        if (!end_bit && out_dev) {
            note_async(c, "Huffman pack");
            return IE_OK;
        }
        HIPCHK(c, hipMemcpyAsync(&end, c->d_chain_end, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        unsigned timeouts = 0;
        if ((r = read_errors(c, &timeouts, nullptr))) return r;
        bool redo;
        if ((r = ticket_redo(c, timeouts, &redo))) return r;
        if (redo) return pack(c, bytes, n, code, len, out, out_cap, start_bit, end_bit);
    }
    if (!out_dev && end > start_bit) {
        const size_t b0 = size_t(start_bit / 8), b1 = size_t((end + 7) / 8);
        HIPCHK(c, hipMemcpy(out + b0, c->d_out + (b0 - size_t(w0) * 4), b1 - b0, hipMemcpyDeviceToHost));
    }
    if (end_bit) *end_bit = end;
    return IE_OK;
}

// `count` strings' histograms and first positions from the device to the caller's arrays (device
// or host; the stream is synchronised for a host array).
int hist_out(ie_ctx* c, uint32_t* hist, uint64_t* first_pos, const void* dh, const void* df, size_t count) {
    const hipMemcpyKind k1 = is_device_ptr(hist) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const hipMemcpyKind k2 = is_device_ptr(first_pos) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(c, hipMemcpyAsync(hist, dh, count * 256 * sizeof(uint32_t), k1, c->stream));
    HIPCHK(c, hipMemcpyAsync(first_pos, df, count * 256 * sizeof(uint64_t), k2, c->stream));
    if (k1 == hipMemcpyDeviceToHost || k2 == hipMemcpyDeviceToHost) HIPCHK(c, hipStreamSynchronize(c->stream));
    return IE_OK;
}

// Walk chunk of the Huffman decode; IE_HUF_CHUNK overrides (tuning aid).  1024 bits measured
// best on a 4K payload (tools/gpu_huf_chunk.sh: 0.30-0.32 ms against 0.34 at 512, 0.37 at 768
// and 2048, 0.55 at 4096)
uint64_t huf_chunk_bits() {
    static const uint64_t huf_chunk = getenv("IE_HUF_CHUNK") ? strtoull(getenv("IE_HUF_CHUNK"), nullptr, 10) : 1024;
    // (at most 2048: the per-chunk symbol counts and middle offsets are u16, and huf_emit_kernel's
    // LDS grows ~33 bytes per chunk bit -- 4096-bit chunks would not fit gfx950's 160 KB)
    return std::min<uint64_t>(2048, std::max<uint64_t>(256, huf_chunk));
}

constexpr size_t kHufBatchBytes = size_t(1) << 30;  // ie_huffman_decode_batch: scratch of one sub-batch

// Scratch of the batched decode under a chunk plan: per image its table entries, chunk entries and
// symbol bases (8-byte words), symbol counts, count-workgroup totals and top-level entries
// (32-bit words); for `batch` images one array per kind, every image's part in turn.
struct HufScratch {
    size_t tab, wg, E, img_bytes;
    size_t base_at, tab_at, count_at, wg_at, e_at, bytes;  // byte offsets for `batch` images
};
HufScratch huf_scratch(size_t nch, size_t batch) {
    HufScratch s;
    s.tab = ie::huffman_batch_tab(int(nch));
    s.wg = ie::huffman_batch_wg(int(nch));
    s.E = ie::huffman_batch_entries();
    s.img_bytes = s.tab * 2 + nch * 16 + (nch + s.wg + s.E) * 4;
    s.base_at = batch * nch * 8;
    s.tab_at = (s.base_at + batch * nch * 8 + 15) / 16 * 16;  // (s.tab is a multiple of 8 entries)
    s.count_at = s.tab_at + batch * s.tab * 2;
    s.wg_at = s.count_at + batch * nch * 4;
    s.e_at = s.wg_at + batch * s.wg * 4;
    s.bytes = s.e_at + batch * s.E * 4;
    return s;
}

// ie_huffman_decode_batch, plus (heads, optional, host) the first head_bytes <= out_pitch bytes
// of every output slot in the same synchronisation: heads + k*head_bytes (the bytes past image
// k's symbols are whatever the slot held).
int huffman_decode_batch(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* len, int count,
                         const uint64_t* start_bit, const uint16_t* lut, uint8_t* out, size_t out_pitch, uint64_t* nout,
                         uint8_t* heads, size_t head_bytes) {
    if (!c) return IE_EINVAL;
    if (!in || !len || !start_bit || !lut || !nout || (!out && out_pitch)) return fail(c, IE_EINVAL, "null argument");
    if (count < 1) return fail(c, IE_EINVAL, "count must be at least 1");
    if (heads && head_bytes > out_pitch) return fail(c, IE_EINVAL, "head_bytes beyond out_pitch");
    const size_t K = size_t(count);
    uint64_t max_span = 0, max_len = 0;
    for (size_t k = 0; k < K; k++) {
        nout[k] = 0;
        if (len[k] > in_pitch)
            return fail(c, IE_EINVAL, "image " + std::to_string(k) + ": len beyond its slot of in_pitch bytes");
        if (start_bit[k] > len[k] * 8) return fail(c, IE_EINVAL, "image " + std::to_string(k) + ": start_bit beyond the stream");
        max_span = std::max(max_span, len[k] * 8 - start_bit[k]);
        max_len = std::max(max_len, len[k]);
    }
    const uint64_t chunk_bits = huf_chunk_bits();
    const uint64_t nch64 = (max_span + chunk_bits - 1) / chunk_bits;
    if (!nch64) return IE_OK;  // every code stream is empty
    if (nch64 > uint64_t(INT32_MAX)) return fail(c, IE_EINVAL, "stream too long for one decode call");
    const size_t nch = size_t(nch64);
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    // the kernels read a stream only through their LDS staging, which stops at its last byte:
    // 4-byte-aligned, 4-byte-pitched device streams are read in place, and device tables too
    const bool in_dev = is_device_ptr(in);
    const uint8_t* src = in;
    size_t pitch = in_pitch;
    if (!in_dev || (reinterpret_cast<uintptr_t>(in) & 3u) || (in_pitch & 3u)) {
        pitch = (size_t(max_len) + 3) / 4 * 4 + 16;
        if ((r = c->d_dec.reserve(c, pitch * K))) return r;
        if (in_dev) {
            HIPCHK(c, hipMemcpy2DAsync(c->d_dec, pitch, in, in_pitch, size_t(max_len), K, hipMemcpyDeviceToDevice, c->stream));
        } else {
            for (size_t k = 0; k < K; k++)
                if (len[k])
                    HIPCHK(c, hipMemcpyAsync(c->d_dec + k * pitch, in + k * in_pitch, size_t(len[k]), hipMemcpyHostToDevice,
                                             c->stream));
        }
        src = c->d_dec;
    }
    const uint16_t* dlut = lut;
    if (!is_device_ptr(lut) || reinterpret_cast<uintptr_t>(lut) % 2) {
        if ((r = c->d_hlut.reserve(c, K * 32768))) return r;
        HIPCHK(c, hipMemcpyAsync(c->d_hlut, lut, K * 32768 * sizeof(uint16_t),
                                 is_device_ptr(lut) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        dlut = c->d_hlut;
    }
    const bool out_dev = is_device_ptr(out);
    uint8_t* dout = out;
    if (!out_dev) {
        if ((r = c->d_hout.reserve(c, K * out_pitch + 1))) return r;
        dout = c->d_hout;
    }
    // the lengths and first bits up, the flag pairs and totals cleared
    if ((r = c->d_hufb_res.reserve(c, 4 * K))) return r;
    if ((r = c->h_hufb_res.reserve(c, 4 * K * sizeof(uint64_t) + K * head_bytes))) return r;
    uint64_t* hres = reinterpret_cast<uint64_t*>(c->h_hufb_res.get());
    uint8_t* hheads = c->h_hufb_res + 4 * K * sizeof(uint64_t);
    for (size_t k = 0; k < K; k++) {
        hres[k] = len[k] * 8;
        hres[K + k] = start_bit[k];
    }
    uint64_t* dres = c->d_hufb_res;
    HIPCHK(c, hipMemcpyAsync(dres, hres, 2 * K * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dres + 2 * K, 0, 2 * K * sizeof(uint64_t), c->stream));
    // per-image scratch; a batch whose scratch would pass kHufBatchBytes runs as sub-batches one
    // after another on the stream (IE_DEC_BATCH_MAX, read on every call, lowers their size further)
    size_t batch = std::max<size_t>(1, kHufBatchBytes / huf_scratch(nch, 1).img_bytes);
    if (const char* eb = getenv("IE_DEC_BATCH_MAX"))
        if (atoi(eb) > 0) batch = std::min<size_t>(batch, size_t(atoi(eb)));
    batch = std::min(batch, K);
    const HufScratch hs = huf_scratch(nch, batch);
    if ((r = c->d_hufb.reserve(c, hs.bytes))) return r;
    ie::HufBatch b{};
    b.nchunks = int(nch);
    b.chunk_bits = chunk_bits;
    b.img_words = pitch / 4;
    b.entry = reinterpret_cast<uint64_t*>(c->d_hufb.get());
    b.base = reinterpret_cast<uint64_t*>(c->d_hufb + hs.base_at);
    b.tab = reinterpret_cast<uint16_t*>(c->d_hufb + hs.tab_at);
    b.count = reinterpret_cast<uint32_t*>(c->d_hufb + hs.count_at);
    b.wgsum = reinterpret_cast<uint32_t*>(c->d_hufb + hs.wg_at);
    b.E = reinterpret_cast<uint32_t*>(c->d_hufb + hs.e_at);
    b.out_pitch = out_pitch;
    for (size_t k0 = 0; k0 < K; k0 += batch) {  // (sub-batches share the scratch: stream order)
        b.images = int(std::min(batch, K - k0));
        b.words = reinterpret_cast<const uint32_t*>(src + k0 * pitch);
        b.nbits = dres + k0;
        b.start_bit = dres + K + k0;
        b.lut = dlut + k0 * 32768;
        b.flags = reinterpret_cast<unsigned*>(dres + 2 * K + k0);
        b.total = dres + 3 * K + k0;
        b.out = dout + k0 * out_pitch;
        if (ie::huffman_decode_images(b, false, c->stream) < 0) return fail(c, IE_EHIP, "Huffman decode walk failed");
        HIPCHK(c, hipGetLastError());
        // the emit follows at once, bounded by out_pitch (a symbol past it is not written and flags
        // its image): no wait for the totals
        ie::huffman_decode_images(b, true, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    // every flag pair and total in ONE read, and the call's one synchronisation
    HIPCHK(c, hipMemcpyAsync(hres + 2 * K, dres + 2 * K, 2 * K * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (heads && head_bytes)
        HIPCHK(c, hipMemcpy2DAsync(hheads, head_bytes, dout, out_pitch, head_bytes, K, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (heads && head_bytes) std::memcpy(heads, hheads, K * head_bytes);
    int code = IE_OK;
    size_t bad = 0;
    bool copied = false;
    for (size_t k = K; k-- > 0;) {
        const uint64_t total = hres[3 * K + k];
        const bool invalid = uint32_t(hres[2 * K + k] >> 32) != 0;
        nout[k] = invalid ? UINT64_MAX : total;
        if (invalid || total > out_pitch) {
            code = invalid ? IE_EFORMAT : IE_ECAP;
            bad = k;
        }
        // a host destination: the symbols of every decodable image, its slot's other bytes untouched
        const size_t nb = size_t(std::min<uint64_t>(total, out_pitch));
        if (!out_dev && !invalid && nb) {
            HIPCHK(c, hipMemcpyAsync(out + k * out_pitch, dout + k * out_pitch, nb, hipMemcpyDeviceToHost, c->stream));
            copied = true;
        }
    }
    if (copied) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (code == IE_EFORMAT)
        return fail(c, code, "image " + std::to_string(bad) + ": Huffman stream holds a bit string no code prefixes");
    if (code == IE_ECAP)
        return fail(c, code, "image " + std::to_string(bad) + ": output capacity below the decoded symbol count");
    return IE_OK;
}

}  // namespace

extern "C" {

int ie_huffman_hist(ie_ctx* c, const uint8_t* bytes, size_t n, uint32_t* hist, uint64_t* first_pos) {
    if (!c || (!bytes && n) || !hist || !first_pos) return IE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    const uint8_t* din;
    if ((r = stage_in(c, bytes, !n || is_device_ptr(bytes), n, &din))) return r;
    HIPCHK(c, hipMemsetAsync(c->d_hist, 0, 256 * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_first, 0xFF, 256 * sizeof(unsigned long long), c->stream));
    if (n) ie::launch_hist(din, n, c->d_hist, c->d_first, reinterpret_cast<unsigned*>(c->d_misc + 3), c->stream);
    HIPCHK(c, hipGetLastError());
    return hist_out(c, hist, first_pos, c->d_hist, c->d_first, 1);
}

int ie_huffman_pack(ie_ctx* c, const uint8_t* bytes, size_t n, const uint32_t* code, const uint8_t* len,
                    uint8_t* out, size_t out_cap, uint64_t start_bit, uint64_t* end_bit) {
    if (!c || (!bytes && n) || !code || !len || !out) return IE_EINVAL;
    return pack(c, bytes, n, code, len, out, out_cap, start_bit, end_bit);
}

int ie_bitcopy(ie_ctx* c, const uint8_t* bytes, size_t n, uint8_t* out, size_t out_cap, uint64_t start_bit) {
    if (!c || (!bytes && n) || !out) return IE_EINVAL;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t end = start_bit + 8 * uint64_t(n);
    const size_t need_bytes = size_t((end + 31) / 32) * 4;  // whole words: the last one is zero-padded
    if (out_cap < need_bytes) return fail(c, IE_ECAP, "output capacity below ceil((start_bit + 8n) / 32) words");
    if (!n) return IE_OK;
    int r;
    const uint8_t* din;
    if ((r = stage_in(c, bytes, is_device_ptr(bytes), n, &din))) return r;
    const uint64_t w0 = start_bit / 32;
    if (is_device_ptr(out)) {
        if (reinterpret_cast<uintptr_t>(out) % 4) return fail(c, IE_EINVAL, "device output must be 4-byte aligned");
        // device to device: asynchronous on the context's stream
        ie::launch_bitshift(din, n, reinterpret_cast<uint32_t*>(out), start_bit, c->stream);
        HIPCHK(c, hipGetLastError());
        if (din == bytes) return IE_OK;
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the staged input must outlive the copy
        return IE_OK;
    }
    // host output: stage from the word holding start_bit (its leading bytes keep the caller's bits)
    if ((r = c->d_out.reserve(c, need_bytes - size_t(w0) * 4))) return r;
    uint8_t word[4] = {0, 0, 0, 0};
    for (int e = 0; e < 4 && size_t(w0) * 4 + e < out_cap; e++) word[e] = out[size_t(w0) * 4 + e];
    HIPCHK(c, hipMemcpyAsync(c->d_out, word, 4, hipMemcpyHostToDevice, c->stream));
    ie::launch_bitshift(din, n, reinterpret_cast<uint32_t*>(c->d_out.get()) - w0, start_bit, c->stream);
    HIPCHK(c, hipGetLastError());
    const size_t b0 = size_t(start_bit / 8), b1 = size_t((end + 7) / 8);
    HIPCHK(c, hipMemcpyAsync(out + b0, c->d_out + (b0 - size_t(w0) * 4), b1 - b0, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IE_OK;
}

int ie_huffman_hist_batch(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* n, int count,
                          uint32_t* hist, uint64_t* first_pos) {
    if (c) c->fused_count = 0;
    if (!c || !in || !n || count <= 0 || !hist || !first_pos) return IE_EINVAL;
    if (!is_device_ptr(in)) return fail(c, IE_EINVAL, "batched Huffman input must be device memory");
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t maxn = 0;
    for (int k = 0; k < count; k++) {
        if (k + 1 < count && n[k] > in_pitch) return fail(c, IE_EINVAL, "string longer than the input pitch");
        maxn = std::max(maxn, n[k]);
    }
    const size_t hb = size_t(count) * 256 * sizeof(uint32_t), fb = size_t(count) * 256 * sizeof(uint64_t);
    const size_t nb = size_t(count) * sizeof(uint64_t), ub = size_t(count) * sizeof(unsigned);
    int r;
    if ((r = c->d_batch.reserve(c, hb + fb + nb + ub))) return r;
    if ((r = c->h_batch.reserve(c, nb))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the pinned staging may still feed a copy
    std::memcpy(c->h_batch, n, nb);
    uint32_t* dh = reinterpret_cast<uint32_t*>(c->d_batch.get());
    auto* df = reinterpret_cast<unsigned long long*>(c->d_batch + hb);
    auto* dn = reinterpret_cast<uint64_t*>(c->d_batch + hb + fb);
    HIPCHK(c, hipMemcpyAsync(dn, c->h_batch, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dh, 0, hb, c->stream));
    HIPCHK(c, hipMemsetAsync(df, 0xFF, fb, c->stream));
    auto* du = reinterpret_cast<unsigned*>(c->d_batch + hb + fb + nb);
    ie::launch_hist_batch(in, in_pitch, dn, maxn, count, dh, df, du, c->stream);
    HIPCHK(c, hipGetLastError());
    return hist_out(c, hist, first_pos, dh, df, size_t(count));
}

int ie_huffman_hist_batch_ends(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* end_bits, int count,
                               uint32_t* hist, uint64_t* first_pos) {
    if (c) c->fused_count = 0;
    if (!c || !in || !end_bits || count <= 0 || !hist || !first_pos) return IE_EINVAL;
    if (!is_device_ptr(in) || !is_device_ptr(end_bits))
        return fail(c, IE_EINVAL, "batched Huffman input and end bits must be device memory");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t hb = size_t(count) * 256 * sizeof(uint32_t), fb = size_t(count) * 256 * sizeof(uint64_t);
    const size_t nb = size_t(count) * sizeof(uint64_t), ub = size_t(count) * sizeof(unsigned);
    int r;
    if ((r = c->d_batch.reserve(c, hb + fb + nb + ub))) return r;
    uint32_t* dh = reinterpret_cast<uint32_t*>(c->d_batch.get());
    auto* df = reinterpret_cast<unsigned long long*>(c->d_batch + hb);
    auto* dn = reinterpret_cast<uint64_t*>(c->d_batch + hb + fb);
    auto* du = reinterpret_cast<unsigned*>(c->d_batch + hb + fb + nb);
    ie::launch_ends_to_bytes(end_bits, uint64_t(in_pitch), count, dn, c->stream, dh, df);
    ie::launch_hist_batch(in, in_pitch, dn, uint64_t(in_pitch), count, dh, df, du, c->stream);
    HIPCHK(c, hipGetLastError());
    return hist_out(c, hist, first_pos, dh, df, size_t(count));
}

int ie_huffman_hist_batch_ends_async(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* end_bits,
                                     int count, int slot) {
    if (!c || !in || !end_bits || count <= 0 || slot < 0 || slot > 1) return IE_EINVAL;
    if (!is_device_ptr(in) || !is_device_ptr(end_bits))
        return fail(c, IE_EINVAL, "batched Huffman input and end bits must be device memory");
    HIPCHK(c, hipSetDevice(c->device));
    // counts left by ie_encode_images_counted for exactly this batch: only the first positions remain
    const bool fused = c->fused_count == count;
    c->fused_count = 0;
    const size_t hb = size_t(count) * 256 * sizeof(uint32_t), fb = size_t(count) * 256 * sizeof(uint64_t);
    const size_t nb = size_t(count) * sizeof(uint64_t), ub = size_t(count) * sizeof(unsigned);
    int r;
    if ((r = c->h_hist[slot].reserve(c, hb + fb + ub))) return r;
    if ((r = c->ev_hist[slot].create(c, hipEventDisableTiming))) return r;
    c->hist_fused[slot] = fused;
    c->hist_in[slot] = in;
    c->hist_pitch[slot] = in_pitch;
    if (fused) {
        // counts from the encoder (cleared as they are read), lengths from the end bits, results
        // straight into the pinned slot: ONE launch, no memset, no copy
        if ((r = c->d_cslot[slot].reserve(c, fb + nb + ub))) return r;
        uint8_t* hp = nullptr;
        if ((r = device_view(c, c->h_hist[slot].get(), &hp))) return r;
        uint8_t* ds = c->d_cslot[slot];
        if ((r = stage_mark(c, 0))) return r;
        ie::launch_first_counted(in, in_pitch, end_bits, uint64_t(in_pitch), count, c->d_chist,
                                 reinterpret_cast<uint64_t*>(ds + fb), reinterpret_cast<unsigned long long*>(ds),
                                 reinterpret_cast<unsigned*>(ds + fb + nb), reinterpret_cast<uint32_t*>(hp),
                                 reinterpret_cast<unsigned long long*>(hp + hb), reinterpret_cast<unsigned*>(hp + hb + fb),
                                 c->stream);
        HIPCHK(c, hipGetLastError());
        c->chist_zero_rows = c->chist_clean_after;  // (the pass cleared rows [0, count))
        if ((r = stage_mark(c, 1))) return r;
        HIPCHK(c, hipEventRecord(c->ev_hist[slot], c->stream));
        c->hist_count[slot] = count;
        return IE_OK;
    }
    if ((r = c->d_batch.reserve(c, hb + fb + nb + ub))) return r;
    uint32_t* dh = reinterpret_cast<uint32_t*>(c->d_batch.get());
    auto* df = reinterpret_cast<unsigned long long*>(c->d_batch + hb);
    auto* dn = reinterpret_cast<uint64_t*>(c->d_batch + hb + fb);
    auto* du = reinterpret_cast<unsigned*>(c->d_batch + hb + fb + nb);
    if ((r = stage_mark(c, 0))) return r;
    ie::launch_ends_to_bytes(end_bits, uint64_t(in_pitch), count, dn, c->stream, dh, df);
    ie::launch_hist_batch(in, in_pitch, dn, uint64_t(in_pitch), count, dh, df, du, c->stream, true);
    HIPCHK(c, hipGetLastError());
    if ((r = stage_mark(c, 1))) return r;
    // histograms and first positions are contiguous on the device: one read-back
    HIPCHK(c, hipMemcpyAsync(c->h_hist[slot], c->d_batch, hb + fb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_hist[slot], c->stream));
    c->hist_count[slot] = count;
    return IE_OK;
}

int ie_huffman_hist_batch_wait(ie_ctx* c, int slot, uint32_t* hist, uint64_t* first_pos) {
    if (!c || slot < 0 || slot > 1 || !hist || !first_pos) return IE_EINVAL;
    if (!c->ev_hist[slot] || !c->hist_count[slot]) return fail(c, IE_EINVAL, "no histogram pending in this slot");
    HIPCHK(c, hipEventSynchronize(c->ev_hist[slot]));
    const int K = c->hist_count[slot];
    const size_t hb = size_t(K) * 256 * sizeof(uint32_t), fb = size_t(K) * 256 * sizeof(uint64_t);
    const size_t nb = size_t(K) * sizeof(uint64_t);
    std::memcpy(hist, c->h_hist[slot], hb);
    std::memcpy(first_pos, c->h_hist[slot] + hb, fb);
    c->hist_count[slot] = 0;
    if (c->hist_fused[slot]) {
        // a string whose first-occurrence scan stopped short (a value first seen past its first
        // 64 chunks): the full pass over the batch, then the device's positions
        const unsigned* un = reinterpret_cast<const unsigned*>(c->h_hist[slot] + hb + fb);
        bool any = false;
        uint64_t maxn = 0;
        for (int k = 0; k < K; k++) any |= un[k] != 0u;
        if (any) {
            uint64_t* nn = reinterpret_cast<uint64_t*>(c->d_cslot[slot] + fb);
            for (int k = 0; k < K; k++) {
                uint64_t s = 0;
                for (int b = 0; b < 256; b++) s += hist[256 * k + b];
                maxn = std::max(maxn, s);
            }
            uint8_t* hp = nullptr;
            if (int r = device_view(c, c->h_hist[slot].get(), &hp)) return r;
            // on the side stream, ordered after the batch's histogram only: work the caller queued on
            // c->stream since _async (e.g. the next batch's encode) is neither waited for nor
            // delayed, and only this launch and its read-back are synchronised
            if (int r = c->tab_stream.create(c, hipStreamNonBlocking)) return r;
            HIPCHK(c, hipStreamWaitEvent(c->tab_stream, c->ev_hist[slot], 0));
            ie::launch_first_full_batch(c->hist_in[slot], c->hist_pitch[slot], nn, maxn, K, reinterpret_cast<const uint32_t*>(hp),
                                        reinterpret_cast<unsigned long long*>(c->d_cslot[slot].get()),
                                        reinterpret_cast<const unsigned*>(c->d_cslot[slot] + fb + nb), c->tab_stream);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(first_pos, c->d_cslot[slot], fb, hipMemcpyDeviceToHost, c->tab_stream));
            HIPCHK(c, hipStreamSynchronize(c->tab_stream));
        }
    }
    return IE_OK;
}

int ie_huffman_pack_batch(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* n, int count,
                          const uint32_t* code, const uint8_t* len, const uint8_t* prefix, size_t prefix_pitch,
                          uint8_t* out, size_t out_pitch, const uint64_t* start_bit, uint64_t* end_bit) {
    if (!c || !in || !n || count <= 0 || !code || !len || !out || !start_bit || (!prefix && prefix_pitch))
        return IE_EINVAL;
    if (!is_device_ptr(in) || !is_device_ptr(out))
        return fail(c, IE_EINVAL, "batched Huffman input and output must be device memory");
    if (reinterpret_cast<uintptr_t>(out) % 4 || out_pitch % 4)
        return fail(c, IE_EINVAL, "output and its pitch must be 4-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    // layout of the staged tables: tiles[count (+1 unused)] n[count] start[count] code[count*256]
    // prefix[count][pw] (words) len[count*256]
    uint64_t pw = 1, ntiles = 0;
    std::vector<uint64_t> ts(size_t(count) + 1);
    unsigned maxlen_all = 0;  // one tile shape for the whole batch
    for (int k = 0; k < count * 256; k++) maxlen_all = std::max<unsigned>(maxlen_all, len[k]);
    const uint64_t tb = uint64_t(ie::pack_tile_bytes(int(maxlen_all)));
    for (int k = 0; k < count; k++) {
        if (k + 1 < count && n[k] > in_pitch) return fail(c, IE_EINVAL, "string longer than the input pitch");
        unsigned maxlen = 0;
        for (int b = 0; b < 256; b++) {
            if (len[256 * k + b] > 32) return fail(c, IE_EINVAL, "code length above 32 bits");
            maxlen = std::max<unsigned>(maxlen, len[256 * k + b]);
        }
        const uint64_t end_bound = start_bit[k] + uint64_t(maxlen) * n[k];
        if (out_pitch < size_t((end_bound + 31) / 32) * 4)
            return fail(c, IE_ECAP, "output pitch below start_bit + max_len * n bits");
        if (start_bit[k] && !prefix) return fail(c, IE_EINVAL, "start_bit > 0 needs a prefix");
        if ((start_bit[k] + 7) / 8 > prefix_pitch && start_bit[k]) return fail(c, IE_EINVAL, "prefix pitch too small");
        pw = std::max<uint64_t>(pw, start_bit[k] / 32 + 1);
        ts[size_t(k)] = (n[k] + tb - 1) / tb;  // tiles of string k
        ntiles = std::max<uint64_t>(ntiles, ts[size_t(k)]);
    }
    ntiles *= uint64_t(count);  // interleaved: tile t -> string t % count (pack_kernel)
    ts[size_t(count)] = 0;
    if (ntiles > uint64_t(INT32_MAX)) return fail(c, IE_EINVAL, "batch too large");
    const size_t K = size_t(count);
    const size_t o_ts = 0, o_n = o_ts + 8 * (K + 1), o_st = o_n + 8 * K, o_code = o_st + 8 * K;
    const size_t o_pre = o_code + 4 * 256 * K, o_len = o_pre + 4 * size_t(pw) * K, total = o_len + 256 * K;
    int r;
    // two pinned staging slots and two device table slots in turn: wait only for this slot's
    // previous copy, not the stream.  The copy runs on a side stream as soon as the tables exist
    // (beside whatever the context's stream is running, e.g. the next batch's encode); the pack
    // waits for it by event, and the copy into a device slot waits for the pack that last read it.
    const int ps = c->pack_slot;
    c->pack_slot ^= 1;
    if (c->pack_recorded[ps]) HIPCHK(c, hipEventSynchronize(c->ev_pack[ps]));
    if ((r = c->h_pack[ps].reserve(c, total))) return r;
    if (c->d_pack[ps].cap() < total && c->d_pack[ps]) HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((r = c->d_pack[ps].reserve(c, total))) return r;
    if ((r = c->ev_pack[ps].create(c, hipEventDisableTiming))) return r;
    if ((r = c->ev_packed[ps].create(c, hipEventDisableTiming))) return r;
    if ((r = c->tab_stream.create(c, hipStreamNonBlocking))) return r;
    uint8_t* h = c->h_pack[ps];
    std::memcpy(h + o_ts, ts.data(), 8 * (K + 1));
    std::memcpy(h + o_n, n, 8 * K);
    std::memcpy(h + o_st, start_bit, 8 * K);
    std::memcpy(h + o_code, code, 4 * 256 * K);
    std::memcpy(h + o_len, len, 256 * K);
    std::memset(h + o_pre, 0, 4 * size_t(pw) * K);
    for (size_t k = 0; k < K; k++) {
        const uint64_t sb = start_bit[k];
        if (!sb) continue;
        uint8_t* d = h + o_pre + 4 * size_t(pw) * k;
        const size_t nbytes = size_t((sb + 7) / 8);
        std::memcpy(d, prefix + k * prefix_pitch, nbytes);
        if (sb % 8) d[nbytes - 1] &= uint8_t(0xFF00u >> (sb % 8));  // bits from start_bit on are the packer's
    }
    if (c->packed_recorded[ps]) HIPCHK(c, hipStreamWaitEvent(c->tab_stream, c->ev_packed[ps], 0));
    HIPCHK(c, hipMemcpyAsync(c->d_pack[ps], h, total, hipMemcpyHostToDevice, c->tab_stream));
    HIPCHK(c, hipEventRecord(c->ev_pack[ps], c->tab_stream));
    c->pack_recorded[ps] = true;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_pack[ps], 0));
    const uint8_t* d = c->d_pack[ps];
    // strings without bytes: the prefix alone
    for (size_t k = 0; k < K; k++)
        if (n[k] == 0)
            HIPCHK(c, hipMemcpyAsync(out + k * out_pitch, d + o_pre + 4 * size_t(pw) * k, 4 * size_t(start_bit[k] / 32 + 1),
                                     hipMemcpyDeviceToDevice, c->stream));
    if (ntiles) {
        if ((r = prepare_state(c, int(ntiles), count))) return r;
        ie::PackArgs a{};
        a.in = in;
        a.code = reinterpret_cast<const uint32_t*>(d + o_code);
        a.len = d + o_len;
        a.ntiles = int(ntiles);
        a.out = reinterpret_cast<uint32_t*>(out);
        a.st = c->d_state;
        a.ticket = c->use_ticket ? c->d_ticket : nullptr;
        a.ticket_base = c->ticket_base;
        a.tag = c->tag;
        a.chain_end = c->d_chain_end;
        a.err = c->d_err;
        a.count = count;
        a.tiles = reinterpret_cast<const uint64_t*>(d + o_ts);
        a.bn = reinterpret_cast<const uint64_t*>(d + o_n);
        a.bstart = reinterpret_cast<const uint64_t*>(d + o_st);
        a.in_pitch = in_pitch;
        a.out_pitch_words = out_pitch / 4;
        a.prefix_pitch_words = pw;
        a.prefix = reinterpret_cast<const uint32_t*>(d + o_pre);
        a.maxlen = int(maxlen_all);
        if ((r = stage_mark(c, 2))) return r;
        ie::launch_pack(a, c->stream);
        if ((r = stage_mark(c, 3))) return r;
        HIPCHK(c, hipGetLastError());
        if (c->use_ticket) c->ticket_base += ntiles;
    }
    HIPCHK(c, hipEventRecord(c->ev_packed[ps], c->stream));  // (the table slot's readers are done)
    c->packed_recorded[ps] = true;
    if (!end_bit) {
        if (ntiles) note_async(c, "Huffman batch pack");
        return IE_OK;
    }
    std::vector<uint64_t> ends(K);
    if (ntiles) HIPCHK(c, hipMemcpyAsync(ends.data(), c->d_chain_end, 8 * K, hipMemcpyDeviceToHost, c->stream));
    unsigned timeouts = 0;
    if ((r = read_errors(c, &timeouts, nullptr))) return r;
    bool redo;
    if ((r = ticket_redo(c, timeouts, &redo))) return r;
    if (redo)
        return ie_huffman_pack_batch(c, in, in_pitch, n, count, code, len, prefix, prefix_pitch, out, out_pitch,
                                     start_bit, end_bit);
    for (size_t k = 0; k < K; k++) end_bit[k] = n[k] ? ends[k] : start_bit[k];
    return IE_OK;
}

int ie_huffman_table(const uint8_t* in, size_t len, uint64_t start_bit, uint16_t* lut, uint64_t* code_start) {
    if ((!in && len) || !lut || !code_start) return IE_EINVAL;
    // MSB-first reads (BitStreamReader::get, BitStream.cpp:14-40); past the end: malformed
    uint64_t pos = start_bit;
    bool over = false;
    auto get = [&](unsigned nb) {
        uint32_t v = 0;
        for (unsigned k = 0; k < nb; k++, pos++) {
            if (pos >= uint64_t(len) * 8) {
                over = true;
                return 0u;
            }
            v = (v << 1) | ((in[pos >> 3] >> (7 - (pos & 7))) & 1u);
        }
        return v;
    };
    // Huffman::buildTree (Huffman.cpp:120-143): groups of {1, count:7, bits:4} headers, each
    // followed by count {key:8, code:bits} entries, ended by a '0' bit; treeAddLeaf (:143-173)
    // grows the tree along the code's bits MSB first (bits = 0 hangs the leaf on the root's left)
    struct Node {
        int child[2] = {-1, -1};
        int sym = -1;
    };
    std::vector<Node> tree(1);
    bool any = false;
    // (an empty stream, or one ending right after its last group, reads as the stop bit)
    while (pos < uint64_t(len) * 8 && get(1)) {
        uint32_t cnt = get(7);
        const uint32_t bl = get(4);
        while (cnt-- && !over) {
            const uint32_t key = get(8), word = get(bl);
            any = true;
            int cur = 0;
            const int steps = bl ? int(bl) : 1;
            for (int b = steps - 1; b >= 0; b--) {
                const int dir = bl ? int((word >> b) & 1u) : 0;
                if (tree[size_t(cur)].child[dir] < 0) {
                    tree[size_t(cur)].child[dir] = int(tree.size());
                    tree.emplace_back();
                }
                cur = tree[size_t(cur)].child[dir];
            }
            tree[size_t(cur)].sym = int(key);
        }
        if (over) return IE_EFORMAT;
    }
    if (over) return IE_EFORMAT;
    *code_start = pos;
    if (!any) return 1;  // no dictionary: the data follows uncompressed (Huffman.cpp:361-371)
    // lut[p] = sym | len << 8 for the leaf the 15-bit string p walks to (codes are <= 15 bits: a
    // 4-bit length field, Huffman.cpp:41-42); 0 where the walk leaves the tree
    constexpr int K = 15;
    std::fill(lut, lut + (size_t(1) << K), uint16_t(0));
    std::vector<std::pair<int, int>> stack{{0, 0}};
    std::vector<uint32_t> path(tree.size(), 0);
    while (!stack.empty()) {
        const auto [nd, depth] = stack.back();
        stack.pop_back();
        const Node& t = tree[size_t(nd)];
        if (t.child[0] < 0 && t.child[1] < 0) {
            if (depth == 0 || depth > K || t.sym < 0) continue;  // a lone root / over-long code: no entry
            const uint32_t lo = path[size_t(nd)] << (K - depth), span = 1u << (K - depth);
            for (uint32_t q = 0; q < span; q++) lut[lo + q] = uint16_t(uint32_t(t.sym) | (uint32_t(depth) << 8));
            continue;
        }
        for (int d = 0; d < 2; d++)
            if (t.child[d] >= 0) {
                path[size_t(t.child[d])] = (path[size_t(nd)] << 1) | uint32_t(d);
                stack.push_back({t.child[d], depth + 1});
            }
    }
    return IE_OK;
}

int ie_huffman_decode(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, const uint16_t* lut,
                      uint8_t* out, size_t out_cap, size_t* nout) {
    if (!c || !in || !lut || !nout) return IE_EINVAL;
    *nout = 0;
    if (start_bit > uint64_t(len) * 8) return fail(c, IE_EINVAL, "start_bit beyond the stream");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    // the kernels read the stream only through their LDS staging, which stops at its last byte: a
    // 4-byte-aligned device stream is read in place, and a device table too (no copies)
    const uint8_t* src = in;
    if (!is_device_ptr(in) || reinterpret_cast<uintptr_t>(in) % 4) {
        const size_t padded = (len + 3) / 4 * 4 + 16;
        if ((r = c->d_dec.reserve(c, padded))) return r;
        if (len)
            HIPCHK(c, hipMemcpyAsync(c->d_dec, in, len, is_device_ptr(in) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                                     c->stream));
        src = c->d_dec;
    }
    const uint16_t* dlut = lut;
    if (!is_device_ptr(lut) || reinterpret_cast<uintptr_t>(lut) % 2) {
        if ((r = c->d_hlut.reserve(c, size_t(32768)))) return r;
        HIPCHK(c, hipMemcpyAsync(c->d_hlut, lut, 32768 * sizeof(uint16_t),
                                 is_device_ptr(lut) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        dlut = c->d_hlut;
    }
    const uint64_t nbits = uint64_t(len) * 8;
    const uint64_t chunk_bits = huf_chunk_bits();
    const size_t nchunks = size_t((nbits - start_bit + chunk_bits - 1) / chunk_bits);
    if (!nchunks) return IE_OK;
    // d_walk: [cap] entries, [cap] symbol bases, then 128 words of top-level entries (256 x u32)
    if ((r = c->d_walk.reserve(c, 2 * nchunks + 130))) return r;
    // per-chunk symbol counts, then the walk workgroups' totals (ie::kTPB chunks each)
    if ((r = c->d_count.reserve(c, nchunks + (nchunks + ie::kTPB - 1) / ie::kTPB + 1))) return r;
    if ((r = c->d_rtab.reserve(c, ie::huffman_table_rows(nbits, start_bit, chunk_bits) + 2))) return r;
    uint64_t* wk = c->d_walk;
    const size_t cap = (c->d_walk.cap() - 130) / 2;
    unsigned* flags = reinterpret_cast<unsigned*>(c->d_misc + 1);
    uint32_t* E = reinterpret_cast<uint32_t*>(wk + 2 * cap);
    // (the flag pair and the total are words [1] and [2]; 48 bytes, a multiple of 16, because a
    // 24-byte fill measured 3 us slower per call: profiles/decode_split_isa.txt)
    HIPCHK(c, hipMemsetAsync(c->d_misc, 0, 6 * sizeof(uint64_t), c->stream));
    const uint32_t* W = reinterpret_cast<const uint32_t*>(src);
    const int rounds = ie::huffman_decode_device(W, nbits, start_bit, dlut, chunk_bits, wk, c->d_rtab, E, c->d_count,
                                                 wk + cap, flags, c->d_misc + 2, nullptr, false, c->stream);
    if (rounds < 0) return fail(c, IE_EHIP, "Huffman decode walk failed");
    HIPCHK(c, hipGetLastError());
    if (is_device_ptr(out)) {
        // device output: the emit follows at once, bounded by out_cap (a symbol past it is not
        // written and flags the launch), and the total and flags come back in ONE read
        ie::huffman_decode_device(W, nbits, start_bit, dlut, chunk_bits, wk, c->d_rtab, E, c->d_count,
                                  wk + cap, flags, c->d_misc + 2, out, true, c->stream, uint64_t(out_cap));
        HIPCHK(c, hipGetLastError());
        uint64_t rb[2] = {0, 0};  // d_misc[1]: the two flag words, d_misc[2]: the total
        HIPCHK(c, hipMemcpyAsync(rb, c->d_misc + 1, sizeof(rb), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *nout = size_t(rb[1]);
        if (uint32_t(rb[0] >> 32)) return fail(c, IE_EFORMAT, "Huffman stream holds a bit string no code prefixes");
        if (rb[1] > out_cap) return fail(c, IE_ECAP, "output capacity below the decoded symbol count");
        return IE_OK;
    }
    uint64_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, c->d_misc + 2, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *nout = size_t(total);
    if (total > out_cap) return fail(c, IE_ECAP, "output capacity below the decoded symbol count");
    // (a host destination from here on: the symbols are emitted into d_hout)
    if ((r = c->d_hout.reserve(c, size_t(total) + 1))) return r;
    uint8_t* dout = c->d_hout;
    ie::huffman_decode_device(W, nbits, start_bit, dlut, chunk_bits, wk, c->d_rtab, E, c->d_count,
                              wk + cap, flags, c->d_misc + 2, dout, true, c->stream);
    HIPCHK(c, hipGetLastError());
    unsigned f[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(f, flags, sizeof(f), hipMemcpyDeviceToHost, c->stream));
    if (total) HIPCHK(c, hipMemcpyAsync(out, dout, size_t(total), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (f[1]) return fail(c, IE_EFORMAT, "Huffman stream holds a bit string no code prefixes");
    return IE_OK;
}

int ie_huffman_decode_batch(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* len, int count,
                            const uint64_t* start_bit, const uint16_t* lut, uint8_t* out, size_t out_pitch, uint64_t* nout) {
    return huffman_decode_batch(c, in, in_pitch, len, count, start_bit, lut, out, out_pitch, nout, nullptr, 0);
}

int ie_huffman_decode_batch_heads(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* len, int count,
                                  const uint64_t* start_bit, const uint16_t* lut, uint8_t* out, size_t out_pitch,
                                  uint64_t* nout, uint8_t* heads, size_t head_bytes) {
    if (!heads) return c ? fail(c, IE_EINVAL, "null argument") : IE_EINVAL;
    return huffman_decode_batch(c, in, in_pitch, len, count, start_bit, lut, out, out_pitch, nout, heads, head_bytes);
}

}  // extern "C"
