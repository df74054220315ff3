// imageencoder_amd/csrc/ie_capi_scaled.cpp -- scaled decode of the C ABI: ie_decode_scaled and
// ie_decode_images_scaled.  The whole stream is parsed and every block transformed as by the full
// decoders; the decode pass stores the rounded means of the pixels over scale x scale cells, so
// w/scale x h/scale bytes per frame are stored and, for a host destination, copied out.  Behind the
// checks the calls are decode_part / decode_images_part (ie_capi_region.cpp).
#include "ie_ctx.hpp"

using namespace iec;

namespace {

// Checks 2-4 of the scaled calls, in the header's order: ie_decode_frames' dimension checks, the
// scale, then the destination's stride and frame pitch against the scaled picture.
int check_scaled(ie_ctx* c, int w, int h, int nframes, int scale, size_t stride, size_t frame_pitch) {
    int r = check_dims(c, w, h, nframes);
    if (r) return r;
    if (scale < 1 || scale > c->n || (scale & (scale - 1)))
        return fail(c, IE_EINVAL, "scale " + std::to_string(scale) + " is not a power of two from 1 to the block size " +
                                      std::to_string(c->n));
    const int ow = w / scale, oh = h / scale;
    if (stride < size_t(ow)) return fail(c, IE_EINVAL, "stride < the scaled width");
    if (nframes > 1 && frame_pitch < frames_span(1, 0, stride, ow, oh))
        return fail(c, IE_EINVAL, "frame_pitch smaller than the scaled frame");
    return IE_OK;
}

PartLaunch scaled_launch(int scale) {
    return [scale](const ie::RecParseArgs& pa, const ie::DecArgs& da, int n, int images, bool batch, hipStream_t s) {
        return ie::launch_rec_parse_decode_scaled(pa, da, n, images, batch, scale, s);
    };
}

}  // namespace

extern "C" {

int ie_decode_scaled(ie_ctx* c, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes, int use_rle,
                     int scale, uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit) {
    if (!c || !in || !out) return IE_EINVAL;
    int r = check_scaled(c, w, h, nframes, scale, stride, frame_pitch);
    if (r) return r;
    return decode_part(c, in, len, start_bit, w, h, nframes, use_rle, w / scale, h / scale, out, stride, frame_pitch, end_bit,
                       scaled_launch(scale));
}

int ie_decode_images_scaled(ie_ctx* c, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                            uint64_t start_bit, int w, int h, int use_rle, int scale, uint8_t* out, size_t stride,
                            size_t frame_pitch, uint64_t* end_bits) {
    if (!c || !in || !nbits || !out) return IE_EINVAL;
    int r = check_scaled(c, w, h, count, scale, stride, frame_pitch);
    if (r) return r;
    return decode_images_part(c, in, in_pitch, nbits, count, start_bit, w, h, use_rle, w / scale, h / scale, out, stride,
                              frame_pitch, end_bits, scaled_launch(scale));
}

}  // extern "C"
