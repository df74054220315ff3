// imageencoder_amd/csrc/ie_capi_region.cpp -- region decode of the C ABI: ie_decode_region and
// ie_decode_images_region.  The whole stream is parsed (chunk plan, scratch and stream staging are
// the full decoders', ie_capi_decode.cpp); only the blocks meeting the rectangle are transformed and
// only the rectangle's pixels are stored and, for a host destination, copied out.  The calls' bodies
// behind their checks -- decode_part and decode_images_part: the parse, a decode pass that writes
// part of every frame, the packed buffer and row copies of a host destination -- are shared with
// the scaled decode (ie_capi_scaled.cpp) through ie_ctx.hpp.
#include "ie_ctx.hpp"

using namespace iec;

namespace {

// Checks 2-4 of the region calls, in the header's order: ie_decode_frames' dimension checks, the
// rectangle, then the destination's stride and frame pitch.
int check_region(ie_ctx* c, int w, int h, int nframes, int x0, int y0, int rw, int rh, size_t stride, size_t frame_pitch) {
    int r = check_dims(c, w, h, nframes);
    if (r) return r;
    if (x0 < 0 || y0 < 0 || rw < 1 || rh < 1 || int64_t(x0) + rw > w || int64_t(y0) + rh > h)
        return fail(c, IE_EINVAL, "rectangle (" + std::to_string(x0) + ", " + std::to_string(y0) + ", " + std::to_string(rw) +
                                      ", " + std::to_string(rh) + ") is empty or not inside the " + std::to_string(w) + "x" +
                                      std::to_string(h) + " frame");
    if (stride < size_t(rw)) return fail(c, IE_EINVAL, "stride < the rectangle's width");
    if (nframes > 1 && frame_pitch < frames_span(1, 0, stride, rw, rh))
        return fail(c, IE_EINVAL, "frame_pitch smaller than the rectangle");
    return IE_OK;
}

// Where the region pass writes: a device `out` in place; for a host one the context's packed buffer
// (rows of rw bytes, rw * rh per frame), whose rows copy_region_out then copies.
struct RegionDest {
    bool out_dev;
    uint8_t* dpix;
    size_t stride, frame_pitch;
};
int region_dest(ie_ctx* c, uint8_t* out, int nframes, int rw, int rh, size_t stride, size_t frame_pitch, RegionDest* d) {
    d->stride = stride;
    d->frame_pitch = frame_pitch;
    const size_t packed = size_t(rw) * size_t(rh);
    int r = pixel_dest(c, c->d_region, out, packed * size_t(nframes), &d->out_dev, &d->dpix);
    if (!d->out_dev) {
        d->stride = size_t(rw);
        d->frame_pitch = packed;
    }
    return r;
}
int copy_region_out(ie_ctx* c, uint8_t* out, const RegionDest& d, int f, int rw, int rh, size_t stride, size_t frame_pitch) {
    HIPCHK(c, hipMemcpy2D(out + size_t(f) * frame_pitch, stride, d.dpix + size_t(f) * d.frame_pitch, d.stride, size_t(rw),
                          size_t(rh), hipMemcpyDeviceToHost));
    return IE_OK;
}

}  // namespace

int iec::decode_part(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes, int use_rle,
                     int rw, int rh, uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit,
                     const PartLaunch& launch) {
    if (start_bit > uint64_t(len) * 8) return fail(c, IE_EINVAL, "start_bit beyond the stream");
    HIPCHK(c, hipSetDevice(c->device));
    const int n = c->n;
    const uint8_t* words;
    int r;
    if ((r = stage_stream_in(c, c->d_dec, in, len, false, &words))) return r;
    const uint64_t nbits = uint64_t(len) * 8;
    const uint64_t nblocks = uint64_t(nframes) * (w / n) * (h / n);
    RecPlan pl{};
    ie::RecParseArgs pa{};
    if ((r = plan_chunks(c, n, nbits - start_bit, nblocks, kMaxChunkBits, &pl))) return r;
    if ((r = dec_scratch(c, n, pl, 1, pa))) return r;
    RegionDest rd;
    if ((r = region_dest(c, out, nframes, rw, rh, stride, frame_pitch, &rd))) return r;
    ie::DecArgs da = dec_args(c, w, h, use_rle, rd.stride);
    da.nframes = nframes;
    da.out = rd.dpix;
    da.frame_pitch = rd.frame_pitch;
    pa.words = reinterpret_cast<const uint32_t*>(words);
    pa.nbits = nbits;
    pa.start_bit = start_bit;
    pa.rle = da.rle;
    if ((r = c->h_decres.reserve(c, 8))) return r;
    pa.total = c->h_decres.dev() + 1;
    pa.end_out = c->h_decres.dev();
    // (as in ie_decode_frames the result words need no clearing: the last chunk's wave always writes
    // the record total, and the end bit is read only when that total covers the last block, whose
    // lane writes it whatever part of the block is stored)
    const int levels = launch(pa, da, n, 1, false, c->stream);
    if (levels < 0) return fail(c, IE_EINVAL, "stream too long for one decode call");
    HIPCHK(c, hipGetLastError());
    c->last_chunks = pa.nchunks;
    c->last_groups = levels;
    c->last_spec = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t end = c->h_decres[0], total = c->h_decres[1];
    if (total < nblocks || end > nbits) return fail(c, IE_EFORMAT, "stream ends before the last block");
    if (!rd.out_dev)
        for (int f = 0; f < nframes; f++)
            if ((r = copy_region_out(c, out, rd, f, rw, rh, stride, frame_pitch))) return r;
    if (end_bit) *end_bit = end;
    return IE_OK;
}

int iec::decode_images_part(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                            uint64_t start_bit, int w, int h, int use_rle, int rw, int rh, uint8_t* out, size_t stride,
                            size_t frame_pitch, uint64_t* end_bits, const PartLaunch& launch) {
    uint64_t max_bits = 0;
    int r;
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
    RegionDest rd;
    if ((r = region_dest(c, out, count, rw, rh, stride, frame_pitch, &rd))) return r;
    ie::DecArgs da = dec_args(c, w, h, use_rle, rd.stride);
    da.nframes = 1;
    da.frame_pitch = rd.frame_pitch;
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
        da.out = rd.dpix + k0 * rd.frame_pitch;
        levels = launch(pa, da, n, m, true, c->stream);
        if (levels < 0) return fail(c, IE_EINVAL, "stream too long for one decode call");
        HIPCHK(c, hipGetLastError());
    }
    c->last_chunks = pl.nchunks;
    c->last_groups = levels;
    c->last_spec = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int bad = -1;
    for (int k = count - 1; k >= 0; k--) {
        const uint64_t end = c->h_imgres[2 * k], total = c->h_imgres[2 * k + 1];
        const bool ok = total >= nblocks && end <= nbits[k];
        if (!ok) bad = k;
        if (end_bits) end_bits[k] = ok ? end : UINT64_MAX;
        if (ok && !rd.out_dev && (r = copy_region_out(c, out, rd, k, rw, rh, stride, frame_pitch))) return r;
    }
    if (bad >= 0) return fail(c, IE_EFORMAT, "image " + std::to_string(bad) + ": stream ends before the last block");
    return IE_OK;
}

extern "C" {

int ie_decode_region(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes, int use_rle,
                     int x0, int y0, int rw, int rh, uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit) {
    if (!c || !in || !out) return IE_EINVAL;
    int r = check_region(c, w, h, nframes, x0, y0, rw, rh, stride, frame_pitch);
    if (r) return r;
    return decode_part(c, in, len, start_bit, w, h, nframes, use_rle, rw, rh, out, stride, frame_pitch, end_bit,
                       [=](const ie::RecParseArgs& pa, const ie::DecArgs& da, int n, int images, bool batch, hipStream_t s) {
                           return ie::launch_rec_parse_decode_region(pa, da, n, images, batch, x0, y0, rw, rh, s);
                       });
}

int ie_decode_images_region(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                            uint64_t start_bit, int w, int h, int use_rle, int x0, int y0, int rw, int rh, uint8_t* out,
                            size_t stride, size_t frame_pitch, uint64_t* end_bits) {
    if (!c || !in || !nbits || !out) return IE_EINVAL;
    int r = check_region(c, w, h, count, x0, y0, rw, rh, stride, frame_pitch);
    if (r) return r;
    return decode_images_part(c, in, in_pitch, nbits, count, start_bit, w, h, use_rle, rw, rh, out, stride, frame_pitch,
                              end_bits,
                              [=](const ie::RecParseArgs& pa, const ie::DecArgs& da, int n, int images, bool batch, hipStream_t s) {
                                  return ie::launch_rec_parse_decode_region(pa, da, n, images, batch, x0, y0, rw, rh, s);
                              });
}

}  // extern "C"
