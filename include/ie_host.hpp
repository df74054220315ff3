// include/ie_host.hpp -- the host-side mirror of the reference's encoder/decoder interface,
// running its block hot path on MI355X through the C-ABI of include/ie_hip.h.
//
// Same class names, constructor arguments, settings keys, bitstream layout and error
// behaviour as the reference (cited per class), so the encoder/decoder CLIs drop onto it:
//   util::BitStreamWriter/Reader  BitStream.hpp:91-171      MSB-first bit IO (header, Huffman dict)
//   dc::ConfigReader              ConfigReader.hpp:41-75    key=value settings file
//   dc::MatrixReader<N>           MatrixReader.hpp:15-37    N x N quantisation matrix (N = 4 or 8)
//   dc::ImageProcessor            ImageBase.hpp:35-77       base of the image encoder / decoder
//   dc::VideoProcessor            VideoBase.hpp:17-48       base of the video encoder / decoder
//   algo::Huffman                 Huffman.hpp:109-142       byte Huffman post-pass (tree on the host)
//   dc::ImageEncoder/ImageDecoder ImageEncoder.hpp, ImageDecoder.hpp
//   dc::VideoEncoder/VideoDecoder VideoEncoder.hpp, VideoDecoder.hpp (any gop: I-frames and
//                                 P-frames with motion compensation on / off, ie_decode_gop; or
//                                 streamed to the output file, ie_vdec)
// Every block-level operation (DCT, quantisation, RLE, bit packing, the inverse) runs on the
// GPU; there is no CPU fallback.
#pragma once

#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "ie_hip.h"

namespace util {

class BitStreamWriter {
public:
    explicit BitStreamWriter(size_t bytes = 0) : buf_(bytes, 0), pos_(0) {}
    void put_bit(int v) { put(1, v ? 1u : 0u); }
    void put(size_t length, uint32_t value);           // low `length` bits, MSB first
    void flush() { pos_ = (pos_ + 7) & ~size_t(7); }  // byte-align (BitStream.cpp:54-59)
    size_t get_position() const { return pos_; }
    size_t get_last_byte_position() const { return (pos_ + 7) / 8; }
    uint8_t* get_buffer() { return buf_.data(); }
    const uint8_t* get_buffer() const { return buf_.data(); }
    std::vector<uint8_t>& bytes() { return buf_; }
    void set_position(size_t p) { pos_ = p; }

private:
    std::vector<uint8_t> buf_;
    size_t pos_;
};

class BitStreamReader {
public:
    BitStreamReader(const uint8_t* b, size_t size) : buf_(b), size_(size), pos_(0) {}
    uint32_t get_bit();                                // 0 past the end (BitStream.cpp:14-28)
    uint32_t get(size_t length);
    size_t get_position() const { return pos_; }
    void set_position(size_t p) { pos_ = p; }
    size_t get_size() const { return size_; }
    size_t get_size_bits() const { return size_ * 8; }
    const uint8_t* get_buffer() const { return buf_; }

private:
    const uint8_t* buf_;
    size_t size_;
    size_t pos_;
};

// Logger (Logger.hpp:12-40): stdout + an append-mode file; "" disables it.
class Logger {
public:
    static void Create(const std::string& file);
    static void Destroy();
    static void WriteLn(const std::string& text);
};

}  // namespace util

namespace dc {

enum class ImageSetting : uint8_t { rawfile = 0, encfile, decfile, rle, quantfile, width, height, logfile, AMOUNT };
enum class VideoSetting : uint8_t {
    rawfile = 0, encfile, decfile, rle, quantfile, width, height, logfile, gop, merange, motioncompensation, AMOUNT
};

// ConfigReader.cpp:75-242 semantics: duplicate keys, missing '=', empty keys are errors; an image
// file has exactly the 8 image keys; a video encoder file has at least the 8 encoder keys.
class ConfigReader {
public:
    bool read(const std::string& fileName);
    bool verifyForImage();
    bool verifyForVideo(bool encoder);
    std::string getValue(ImageSetting key) const;
    std::string getValue(VideoSetting key) const;
    std::string getErrorDescription() const { return err_; }
    std::string toString() const;

private:
    std::map<std::string, std::string> kv_;
    std::string err_;
};

// The reference's default block size (Block.hpp:13); the GPU library takes 4 or 8 at run time.
static constexpr uint16_t BlockSize = 4u;

// dc::MatrixReader<size> (MatrixReader.hpp:15-37, MatrixReader.cpp:46-198): a size x size
// quantisation matrix read from whitespace-separated text (the reference's acceptance rules and
// messages), written to the stream as a 5-bit width followed by size*size values of that width.
// getData() is the matrix as doubles, as the reference hands it to Block<>::processDCTDivQ;
// data() the uint16 values for ie_set_quant.  Instantiated for 4 and 8 (config.cpp).
template <size_t size = BlockSize>
class MatrixReader {
public:
    MatrixReader();
    static MatrixReader<size> fromBitstream(util::BitStreamReader& reader);
    bool read(const std::string& fileName);
    void write(util::BitStreamWriter& writer) const;
    const std::string toString() const;
    uint8_t getMaxBitLength() const;
    const double* getData() const { return expanded_; }
    const uint16_t* data() const { return matrix_; }
    static constexpr size_t SIZE_LEN_BITS = 5;

private:
    uint16_t matrix_[size * size];
    double expanded_[size * size];
};

// What an encoder keeps of its MatrixReader<N>: the block size (a run-time parameter of the GPU
// library) and the matrix values.
struct QuantSpec {
    int n = 0;
    std::vector<uint16_t> q;
    template <size_t N>
    static QuantSpec from(const MatrixReader<N>& m) {
        QuantSpec s;
        s.n = int(N);
        s.q.assign(m.data(), m.data() + N * N);
        return s;
    }
};

}  // namespace dc

namespace algo {

// Huffman<uint8_t> (Huffman.cpp:233-402).  encode(): device histogram + first occurrence, the
// tree / dictionary replayed on the host with the reference's own libstdc++ containers, device
// re-encode.  decode(): dictionary and tree on the host, the bit walk on the device.
class Huffman {
public:
    // Encode `n` bytes at `in` (host or device).  Returns the output bytes (host).  `ctx` runs
    // the device stages.
    static int encode(ie_ctx* ctx, const uint8_t* in, size_t n, std::vector<uint8_t>& out);
    // Decode a stream that starts with the Huffman flag bit.  passthrough = true: no table, the
    // payload starts at *start_bit of `in` itself; else `out` receives the decoded bytes (the bit
    // walk runs on ctx's device, ie_huffman_decode).  Returns IE_OK or an ie_hip.h error code.
    // The dictionary part alone: the 15-bit prefix table ie_huffman_decode walks with (lut: 32768
    // entries), and where the code stream starts; passthrough when the stream holds no dictionary.
    static int decode_table(const uint8_t* in, size_t n, uint16_t* lut, bool& passthrough, size_t& start_bit);
    static int decode(ie_ctx* ctx, const uint8_t* in, size_t n, std::vector<uint8_t>& out, bool& passthrough,
                      size_t& start_bit);
};

}  // namespace algo

namespace dc {

// Owns one device context; one per process is enough for the CLIs.
class Device {
public:
    static ie_ctx* get();
};

// dc::ImageProcessor (ImageBase.hpp:35-77): the image encoder / decoder base.  The encoder
// constructor takes (source, dest, width, height, use_rle, quant matrix) and reads the raw file
// (ImageBase.cpp:19-30, 78-88); the decoder constructor takes (source, dest) and learns every
// setting from the stream (ImageBase.cpp:98-129).  process() / saveResult() are the reference's
// virtual pair.  Where the reference builds one heap Block<> per block (ImageBase.cpp:175-206)
// and loops over them, process() here hands the whole frame to the GPU library: dc::Block<N>
// has no counterpart -- see DESIGN.md §1.
class ImageProcessor {
public:
    ImageProcessor(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                   const uint16_t& height, const bool& use_rle, MatrixReader<>& quant_m)
        : ImageProcessor(source_file, dest_file, width, height, use_rle, QuantSpec::from(quant_m)) {}
    template <size_t N>
    ImageProcessor(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                   const uint16_t& height, const bool& use_rle, MatrixReader<N>& quant_m)
        : ImageProcessor(source_file, dest_file, width, height, use_rle, QuantSpec::from(quant_m)) {}
    ImageProcessor(const std::string& source_file, const std::string& dest_file);
    virtual ~ImageProcessor() = default;

    virtual bool process() = 0;
    virtual void saveResult() const {}

    const std::vector<uint8_t>& result() const { return result_; }  // encoded file / decoded pixels
    std::string error() const { return err_; }
    uint16_t getWidth() const { return width; }
    uint16_t getHeight() const { return height; }

    static constexpr size_t RLE_BITS = 1u;   // ImageBase.hpp:75
    static constexpr size_t DIM_BITS = 15u;  // ImageBase.hpp:76

protected:
    ImageProcessor(const std::string& source_file, const std::string& dest_file, uint16_t width, uint16_t height,
                   bool use_rle, QuantSpec quant);
    void saveResult(bool encoded) const;  // ImageBase.cpp:309-330: the file and the size report

    uint16_t width = 0, height = 0;
    bool use_rle = true;
    QuantSpec quant_m;
    std::string source_file, dest_file;
    std::vector<uint8_t> raw;      // the input file (ImageBase::raw)
    std::vector<uint8_t> result_;  // what saveResult writes
    std::string err_;
};

struct EncodeOptions {
    bool huffman = true;   // the reference's ENABLE_HUFFMAN (makefile:13)
    int mode = IE_MODE_FAST;
};

// dc::ImageEncoder (ImageEncoder.hpp:12-23, ImageEncoder.cpp:19-180).
class ImageEncoder : public ImageProcessor {
public:
    ImageEncoder(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                 const uint16_t& height, const bool& use_rle, MatrixReader<>& m, EncodeOptions opt = EncodeOptions())
        : ImageProcessor(source_file, dest_file, width, height, use_rle, m), opt_(opt) {}
    template <size_t N>
    ImageEncoder(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                 const uint16_t& height, const bool& use_rle, MatrixReader<N>& m, EncodeOptions opt = EncodeOptions())
        : ImageProcessor(source_file, dest_file, width, height, use_rle, m), opt_(opt) {}
    bool process() override;
    void saveResult() const override { ImageProcessor::saveResult(true); }

private:
    EncodeOptions opt_;
};

// dc::ImageDecoder (ImageDecoder.hpp:11-21, ImageDecoder.cpp:17-129).  The block size of the
// stream is the reference's compile-time BlockSize; here block_size (0: IE_BLOCKSIZE, default 4).
class ImageDecoder : public ImageProcessor {
public:
    ImageDecoder(const std::string& source_file, const std::string& dest_file, int block_size = 0);
    bool process() override;
    void saveResult() const override { ImageProcessor::saveResult(false); }
    uint16_t width_px() const { return width; }

private:
    int n_;
};

// dc::VideoProcessor (VideoBase.hpp:17-48): the video encoder / decoder base; frames are YUV420
// (Y + W*H/2 bytes, VideoBase.cpp:6-19).  The payloads follow a 210-bit header bit-contiguously
// (VideoEncoder.cpp:22-107, Frame.cpp:31-45).  Any gop: frame f is an I-frame when f % gop == 0,
// every other frame a P-frame (motion search + coded prediction error).  The encoder streams the
// file through an ie_vstream for every gop (with gop > 1 in chunks of whole groups of pictures,
// ie_vstream_open_gop) and never holds the whole video; the decoder reads the ENCODED file whole
// and, with stream_to_file (the decoder command line), hands the decoded frames to the output file
// chunk by chunk through an ie_vdec, so it never holds the decoded video either.
class VideoProcessor {
public:
    VideoProcessor(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                   const uint16_t& height, const bool& use_rle, MatrixReader<>& quant_m, const uint16_t& gop,
                   const uint16_t& merange)
        : VideoProcessor(source_file, dest_file, width, height, use_rle, QuantSpec::from(quant_m), gop, merange) {}
    template <size_t N>
    VideoProcessor(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                   const uint16_t& height, const bool& use_rle, MatrixReader<N>& quant_m, const uint16_t& gop,
                   const uint16_t& merange)
        : VideoProcessor(source_file, dest_file, width, height, use_rle, QuantSpec::from(quant_m), gop, merange) {}
    VideoProcessor(const std::string& source_file, const std::string& dest_file, const bool& motioncomp);
    virtual ~VideoProcessor() = default;

    virtual bool process() = 0;
    virtual void saveResult() const {}

    const std::vector<uint8_t>& result() const { return result_; }
    std::string error() const { return err_; }

protected:
    VideoProcessor(const std::string& source_file, const std::string& dest_file, uint16_t width, uint16_t height,
                   bool use_rle, QuantSpec quant, uint16_t gop, uint16_t merange);
    void saveResult(bool encoded) const;

    uint16_t width = 0, height = 0, gop = 1, merange = 0;
    bool use_rle = true, motioncomp = false;
    QuantSpec quant_m;
    std::string source_file, dest_file;
    // the decoder reads its (encoded) input whole; the encoder STREAMS its .raw/YUV420 input
    // (VideoEncoder::process reads it frame chunk by frame chunk), so raw stays empty there
    std::vector<uint8_t> raw, result_;
    size_t raw_size = 0;  // input file size
    std::string err_;
};

// dc::VideoEncoder (VideoEncoder.hpp:11-21).
class VideoEncoder : public VideoProcessor {
public:
    VideoEncoder(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                 const uint16_t& height, const bool& use_rle, MatrixReader<>& m, const uint16_t& gop,
                 const uint16_t& merange, EncodeOptions opt = EncodeOptions())
        : VideoProcessor(source_file, dest_file, width, height, use_rle, m, gop, merange), opt_(opt) {}
    template <size_t N>
    VideoEncoder(const std::string& source_file, const std::string& dest_file, const uint16_t& width,
                 const uint16_t& height, const bool& use_rle, MatrixReader<N>& m, const uint16_t& gop,
                 const uint16_t& merange, EncodeOptions opt = EncodeOptions())
        : VideoProcessor(source_file, dest_file, width, height, use_rle, m, gop, merange), opt_(opt) {}
    bool process() override;
    void saveResult() const override { VideoProcessor::saveResult(true); }

private:
    EncodeOptions opt_;
};

// dc::VideoDecoder (VideoDecoder.hpp): frames of Y + W*H/2 bytes of 0x80 (Frame.cpp:121-124).
// stream_to_file: process() decodes through an ie_vdec and writes dest_file chunk by chunk as the
// frames arrive (two chunks of frames on the device, one on the host, whatever the video's length);
// result() stays empty, saveResult() only logs, and a failure removes the partial file.
class VideoDecoder : public VideoProcessor {
public:
    VideoDecoder(const std::string& source_file, const std::string& dest_file, const bool& motioncomp,
                 int block_size = 0, bool stream_to_file = false);
    bool process() override;
    void saveResult() const override;

private:
    bool processToFile();
    int n_;
    bool stream_to_file_;
};

}  // namespace dc

// C entry points of the host library (Python bindings, tests, bench).
extern "C" {
// The settings header alone (ImageEncoder.cpp:84-94; video adds frame_count, gop, merange,
// VideoEncoder.cpp:60-73) into out (host, zeroed by this call).  Returns its length in BITS.
int64_t ieh_write_header(uint8_t* out, size_t cap, int n, const uint16_t* q, int rle, int w, int h, int huffman,
                         int video, int frames, int gop, int merange);
// Whole image file as the reference encoder writes it (header + blocks [+ Huffman pass]).
// y: host or device; out: host.  Returns bytes written, < 0 on error.
int64_t ieh_encode_image(ie_ctx* ctx, const uint8_t* y, int w, int h, const uint16_t* q, int n, int rle,
                         int huffman, int mode, uint8_t* out, size_t cap);
// ---- Rate control by scaling the quantisation matrix (the matrix travels in the file's header, so
// a file written with any matrix is a valid file for the reference decoder).
// out[k] = clamp((base[k] * percent + 50) / 100, 1, 65535) in 64-bit integer arithmetic; percent >= 1
// (IE_EINVAL otherwise, and for n not 4 or 8).  No GPU involved.
int ieh_scale_matrix(const uint16_t* base, int n, int percent, uint16_t* out);
// The 32 percents the budget search probes first: round(100 * 2^(j/4)), j = -8 .. 23 (25 .. 5382),
// into out (optional).  Returns 32.
int ieh_budget_ladder(int* out);
// Whole image file (as ieh_encode_image writes it) with the FINEST probed scale of `base` whose
// file fits budget_bytes.  Returns the bytes written, *percent = the scale chosen.
//  - The size judged is ceil((header bits + payload bits) / 8) BEFORE any Huffman pass: the header
//    as ieh_write_header writes it for the scaled matrix (its length depends on the matrix's widest
//    value), the payload from ie_probe_sizes.  With huffman = 1 the chosen matrix then goes through
//    the normal ieh_encode_image path and the file is whatever that yields: usually smaller, in the
//    reference's "no gain" case (Huffman.cpp:329-341) those bytes plus one bit, so possibly one
//    byte over the budget.
//  - Size is not monotone in the scale (the matrix, the quotients and the header width are all
//    rounded), so the search does not bisect: ONE ie_probe_sizes call over the ladder above (distinct
//    matrices only); p1 = the smallest ladder percent that fits, p0 the entry below it; ONE more call
//    over the integers p0 + ceil(i (p1 - p0) / 33), i = 1 .. 32, strictly between the two; the result
//    is the smallest percent of both sets that fits.  p1 = 25 ends the search at once.
//  - Nothing fits: IE_ECAP, *percent = 5382, nothing written, ie_last_error "no scale up to 5382 %
//    meets the budget" (the context's matrix is then `base`).  Otherwise the context's matrix is the
//    chosen one.  IE_ECAP with another message: cap is below the file.
//  - IE_EDEVICE if the encoded file's size before the Huffman pass ever differs from the probed one.
int64_t ieh_encode_image_budget(ie_ctx* ctx, const uint8_t* y, int w, int h, const uint16_t* base, int n, int rle,
                                int huffman, int mode, size_t budget_bytes, uint8_t* out, size_t cap, int* percent);
// Whole image file (as ieh_encode_image writes it) with the COARSEST probed scale of `base` whose
// distortion -- the squared error of the decoded pixels against y, ie_probe_rd -- is at most
// max_sse.  Returns the bytes written, *percent = the scale chosen, *sse = its distortion.
//  - Distortion is no more monotone in the scale than size is, so the search mirrors the budget
//    search: ONE ie_probe_rd call over the ladder (distinct matrices only); p0 = the largest ladder
//    percent with sse <= max_sse, p1 the entry above it; ONE more call over the integers
//    p0 + ceil(i (p1 - p0) / 33), i = 1 .. 32, strictly between the two; the result is the largest
//    percent of both sets that meets max_sse.  p0 = 5382 ends the search at once.
//  - Nothing meets it: IE_ECAP, *percent = 25, nothing written, ie_last_error "no scale down to
//    25 % meets the quality" (the context's matrix is then `base`).  Otherwise the context's matrix
//    is the chosen one.  IE_ECAP with another message: cap is below the file.
//  - IE_EDEVICE if the encoded file's size before the Huffman pass differs from the probed one (the
//    sizes come along in the same probe calls).
int64_t ieh_encode_image_quality(ie_ctx* ctx, const uint8_t* y, int w, int h, const uint16_t* base, int n,
                                 int rle, int huffman, int mode, uint64_t max_sse, uint8_t* out, size_t cap,
                                 int* percent, uint64_t* sse);
// gop=1 video file from a YUV420 buffer (frame_count = len / (1.5 w h)).
int64_t ieh_encode_video(ie_ctx* ctx, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* q, int n,
                         int rle, int huffman, int merange, int mode, uint8_t* out, size_t cap);
// Video file with I/P-frames: frame f is an I-frame when f % gop == 0 (VideoEncoder.cpp:22-107; the
// P-frames' motion search + coded error through ie_encode_gop_groups).  gop = 1: ieh_encode_video.
int64_t ieh_encode_video_gop(ie_ctx* ctx, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* q, int n,
                             int rle, int huffman, int gop, int merange, int mode, uint8_t* out, size_t cap);
// Whole video file (exactly as ieh_encode_video_gop writes it) with the FINEST probed scale of `base`
// whose file fits budget_bytes: ieh_encode_image_budget's contract, search, error codes and messages
// for a video.  The size judged is ceil((video header bits for the scaled matrix + the bits of all
// frames) / 8) before any Huffman pass, the frames' bits from ie_probe_gop (one call over the
// ladder's distinct matrices, one over the refinement).  The frames lie 1.5 w h bytes apart and
// only Y is read; host frames go to the device once, for the probes and the encode.
int64_t ieh_encode_video_budget(ie_ctx* ctx, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* base,
                                int n, int rle, int huffman, int gop, int merange, int mode, size_t budget_bytes,
                                uint8_t* out, size_t cap, int* percent);
// Whole video file (exactly as ieh_encode_video_gop writes it) with the COARSEST probed scale of
// `base` whose distortion is at most max_sse: ieh_encode_image_quality's contract, search, error
// codes, messages and context state for a video.  The distortion judged is the sum over all frames
// of ie_probe_gop_rd's sse (Y planes only) for the decoder setting `motioncomp`; the sizes come
// along in the same two probe calls.  *sse: the chosen scale's total; frame_sse (optional): its
// error of every frame, len / (1.5 w h) entries -- the total hides that the late frames of a group
// drift worst.  The frames lie 1.5 w h bytes apart; host frames go to the device once, for both
// probes and the encode.  What ie_probe_gop_rd refuses (P-frames with W or H no multiple of 16, or
// with 8x8 blocks) is IE_EINVAL here.
int64_t ieh_encode_video_quality(ie_ctx* ctx, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* base,
                                 int n, int rle, int huffman, int gop, int merange, int motioncomp, int mode,
                                 uint64_t max_sse, uint8_t* out, size_t cap, int* percent, uint64_t* sse,
                                 uint64_t* frame_sse);
// Decode an image file (host buffer) with block size n: pixels into out (w*h bytes).  A cap
// below w*h returns IE_ECAP with *w / *h set, right after the header (the payload is not decoded):
// call with cap = 0 to size the buffer.
int64_t ieh_decode_image(ie_ctx* ctx, const uint8_t* enc, size_t len, int n, uint8_t* out, size_t cap, int* w,
                         int* h);
// Decode only the rectangle (x0, y0, rw, rh) of an image file (as ieh_encode_image writes it, with
// or without the Huffman pass): the front half of ieh_decode_image -- Huffman pass, settings header,
// ie_set_quant with the header's matrix -- then ie_decode_region.  out (host or device) receives
// rw*rh bytes, rows packed; they equal that crop of what ieh_decode_image writes.  Returns the
// bytes written.  *w / *h: the header's size, set whenever the header was read.  A rectangle that
// does not fit it is IE_EINVAL (nothing is decoded), cap < rw*rh IE_ECAP.
int64_t ieh_decode_image_region(ie_ctx* ctx, const uint8_t* enc, size_t len, int n, int x0, int y0, int rw, int rh,
                                uint8_t* out, size_t cap, int* w, int* h);
// Decode an image file at 1/scale of its width and height (scale = 1, 2, 4 or 8, at most n): the
// front half of ieh_decode_image_region, then ie_decode_scaled.  out (host or device) receives
// ow*oh bytes, ow = w/scale, oh = h/scale, rows packed: the rounded box means of what
// ieh_decode_image writes.  Returns the bytes written.  *w / *h: the header's full size, set
// whenever the header was read.  A bad scale is IE_EINVAL (nothing is decoded), cap < ow*oh IE_ECAP.
int64_t ieh_decode_image_scaled(ie_ctx* ctx, const uint8_t* enc, size_t len, int n, int scale, uint8_t* out, size_t cap,
                                int* w, int* h);
/* Decode `count` image files that share their settings (quant matrix, rle, w, h) with block size n:
 * file k is len[k] bytes at enc + k*enc_pitch (host memory); the pixels, w*h bytes per image back to
 * back in file order, go to out (host or device, cap bytes).  Returns the pixel bytes, < 0 on error.
 *  - Huffman-coded files: the dictionaries are parsed on the host (ie_huffman_table), ONE
 *    ie_huffman_decode_batch call decodes every file into device slots, and ONE ie_decode_images
 *    call reads those slots in place: the decoded streams never cross to the host, except the
 *    first 256 bytes of each (its settings header), which ride with the symbol counts.  Two
 *    synchronisations per call (plus ie_set_quant's when the matrix differs from the context's).
 *  - Files without a dictionary (the "no gain" output, Huffman.cpp:329-341) form a second group,
 *    read by ie_decode_images straight from the file bytes; a batch may mix both kinds.
 *  - IE_EINVAL when a file's settings differ from file 0's; IE_EFORMAT for a malformed or truncated
 *    file; ie_last_error names the file ("file k: ...").
 *  - A cap below count*w*h returns IE_ECAP with *w / *h set, after the headers are known and before
 *    any record decode (ieh_decode_image's convention). */
int64_t ieh_decode_images(ie_ctx* ctx, const uint8_t* enc, size_t enc_pitch, const uint64_t* len, int count, int n,
                          uint8_t* out, size_t cap, int* w, int* h);
// Decode a gop=1 video file: frames of Y + w*h/2 bytes of 0x80 (Frame.cpp:121-124).  A cap
// below the frames' size returns IE_ECAP after the header, as ieh_decode_image.
int64_t ieh_decode_video(ie_ctx* ctx, const uint8_t* enc, size_t len, int n, uint8_t* out, size_t cap, int* w,
                         int* h, int* frames);
// The same file decoded chunk by chunk (ie_vdec over the payload; ie_hip.h): open runs the Huffman
// pass, reads the header (returned through w .. merange) and ie_set_quant, and opens the decoder
// (chunk_frames as ie_vdec_open; enc may be freed when it returns); next writes whole frames in the
// file's layout -- Y, then w*h/2 bytes of 0x80 -- into out (host memory), as many as cap holds and
// the video has left (*got; 0 at the end); the frames in order are ieh_decode_video's bytes.  A
// truncated file: the frames before the cut, then IE_EFORMAT (ie_vdec_next's contract).
typedef struct ieh_vdec ieh_vdec;
int ieh_vdec_open(ie_ctx* ctx, const uint8_t* enc, size_t len, int n, int motioncomp, int chunk_frames, int* w, int* h,
                  int* frames, int* gop, int* merange, ieh_vdec** out);
int ieh_vdec_next(ieh_vdec* v, uint8_t* out, size_t cap, int* got);
int ieh_vdec_close(ieh_vdec* v);
// Huffman post-pass entirely between device buffers (in, out device memory; out needs
// ~n + 4 KiB).  Returns output bytes; only the 256-entry histogram and code table cross PCIe.
int64_t ieh_huffman_encode_device(ie_ctx* ctx, const uint8_t* din, size_t n, uint8_t* dout, size_t cap);
/* Batched device Huffman pass: string k = n[k] bytes at din + k*in_pitch -> dout + k*out_pitch
 * (device memory; out_pitch 4-byte aligned and >= the loose bound (dict + max_len * n[k]) / 8).
 * bytes[k] receives each output length.  The outputs are complete when the context's stream is. */
int ieh_huffman_encode_device_batch(ie_ctx* ctx, const uint8_t* din, size_t in_pitch, const uint64_t* n, int count,
                                    uint8_t* dout, size_t out_pitch, int64_t* bytes);
// Free the host library's device scratch for ctx (call before ie_destroy).
void ieh_release(ie_ctx* ctx);
// Huffman post-pass of n bytes (host or device) into out (host).  Returns output bytes.
int64_t ieh_huffman_encode(ie_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out, size_t cap);
// Batched Huffman pass over the images of the last ie_encode_images launch on ctx (device output
// at din + k*in_pitch), lengths from the encoder's end bits on the device; bytes[k] = output size.
int ieh_huffman_encode_after_encode(ie_ctx* ctx, const uint8_t* din, size_t in_pitch, int count, uint8_t* dout,
                                    size_t out_pitch, int64_t* bytes);
// The same in two halves for pipelining batches (slot 0 / 1 alternating): _begin launches the
// histogram and returns; _finish waits for it, builds the trees and launches the pack.
int ieh_huffman_begin_after_encode(ie_ctx* ctx, const uint8_t* din, size_t in_pitch, int count, int slot);
int ieh_huffman_finish_after_encode(ie_ctx* ctx, const uint8_t* din, size_t in_pitch, int count, int slot,
                                    uint8_t* dout, size_t out_pitch, int64_t* bytes);
// Huffman<uint8_t>::decode alone (Huffman.cpp:354-402; the bit walk on the device): decoded byte
// count, or 0 with *passthrough = 1 when the stream has no dictionary.
int64_t ieh_huffman_decode(ie_ctx* ctx, const uint8_t* in, size_t n, uint8_t* out, size_t cap, int* passthrough);
// The dictionary of a Huffman-coded stream (host bytes) as ie_huffman_decode's 15-bit prefix table
// (lut: 32768 entries) and the code stream's first bit: a caller with the stream in device memory
// then decodes it device-resident.  Returns 1 when there is no dictionary (passthrough), 0, or < 0.
int ieh_huffman_table(const uint8_t* in, size_t n, uint16_t* lut, uint64_t* start_bit);
}
