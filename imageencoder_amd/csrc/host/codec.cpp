// imageencoder_amd/csrc/host/codec.cpp -- file-level encoders/decoders over the GPU codec:
// the settings header on the host (ImageEncoder.cpp:84-94, VideoEncoder.cpp:60-73), block
// records by ie_encode_frames straight behind it in device memory, the optional Huffman pass on
// the device bytes, one copy of the finished file to the host.  Decoding mirrors
// ImageProcessor(source, dest) (ImageBase.cpp:90-125) + ImageDecoder::process.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <utility>

#include "host_internal.hpp"
#include "ie_host.hpp"

namespace dc {

bool is_device(ie_ctx*, const void* p) { return ie_is_device_ptr(p) != 0; }

struct Scratch {
    DeviceBuffer enc, huf, pix;
    explicit Scratch(ie_ctx* c) : enc(c), huf(c), pix(c) {}
};
std::mutex g_mu;
std::map<ie_ctx*, std::unique_ptr<Scratch>> g_scratch;

Scratch& scratch(ie_ctx* c) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto& s = g_scratch[c];
    if (!s) s.reset(new Scratch(c));
    return *s;
}

namespace {

bool read_file(const std::string& name, std::vector<uint8_t>& out) {
    std::ifstream f(name, std::ios::binary);
    if (!f) return false;
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

bool write_file(const std::string& name, const std::vector<uint8_t>& data) {
    std::ofstream f(name, std::ios::binary | std::ios::trunc);
    if (!f) return false;
    f.write(reinterpret_cast<const char*>(data.data()), std::streamsize(data.size()));
    return bool(f);
}

int block_size_from_env() {
    const char* e = std::getenv("IE_BLOCKSIZE");
    return (e && std::atoi(e) == 8) ? 8 : 4;
}

std::string fmt(const char* f, double a, double b = 0, double c = 0) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), f, a, b, c);
    return buf;
}

FileParams image_params(int w, int h, int n, const uint16_t* q, bool rle, bool huffman, int mode) {
    FileParams p;
    p.w = w;
    p.h = h;
    p.n = n;
    p.q = q;
    p.rle = rle;
    p.huffman = huffman;
    p.mode = mode;
    return p;
}

// A video of `len` bytes of Y + UV frames (VideoBase.cpp:8-9); false unless it holds 1..32767 of them
bool video_params(int w, int h, int n, const uint16_t* q, bool rle, bool huffman, int mode, size_t len, int gop,
                  int merange, FileParams* p) {
    *p = image_params(w, h, n, q, rle, huffman, mode);
    p->video = true;
    p->frame_pitch = size_t(w) * h + size_t(w) * h / 2;
    p->frames = int(std::min<size_t>(p->frame_pitch ? len / p->frame_pitch : 0, 32768));  // (no wrap-around into range)
    p->gop = gop < 1 ? 1 : gop;
    p->merange = merange;
    return p->frames > 0 && p->frames <= 32767;
}

}  // namespace

ie_ctx* Device::get() {
    static ie_ctx* ctx = [] {
        ie_ctx* c = nullptr;
        const char* d = std::getenv("IE_DEVICE");
        if (ie_create(d ? std::atoi(d) : 0, &c) != IE_OK) return static_cast<ie_ctx*>(nullptr);
        return c;
    }();
    return ctx;
}

void write_header(util::BitStreamWriter& hdr, const FileParams& p) {
    // settings header (Huffman off: a leading '0' bit, ImageEncoder.cpp:84-86)
    if (!p.huffman) hdr.put_bit(0);
    const uint16_t* qv = p.q;  // MatrixReader::write (MatrixReader.cpp:145-158)
    int qb = 0;
    for (int k = 0; k < p.n * p.n; k++) qb = std::max(qb, qv[k] ? 32 - __builtin_clz(uint32_t(qv[k])) : 1);
    hdr.put(5, uint32_t(qb));
    for (int k = 0; k < p.n * p.n; k++) hdr.put(size_t(qb), qv[k]);
    hdr.put(1, p.rle ? 1u : 0u);  // ImageEncoder.cpp:92-94
    hdr.put(15, uint32_t(p.w));
    hdr.put(15, uint32_t(p.h));
    if (p.video) {  // VideoEncoder.cpp:71-73
        hdr.put(15, uint32_t(p.frames));
        hdr.put(15, uint32_t(p.gop));
        hdr.put(15, uint32_t(p.merange));
    }
}

int encode_file(ie_ctx* c, const uint8_t* y, const FileParams& p, std::vector<uint8_t>& out, std::string& err,
                size_t* pre_bytes) {
    if (!c) return (err = "no GPU context", IE_EHIP);
    int r;
    if ((r = ie_set_quant(c, p.q, p.n))) return (err = ie_last_error(c), r);
    util::BitStreamWriter hdr(64);
    write_header(hdr, p);
    const uint64_t H = hdr.get_position();

    Scratch& s = scratch(c);
    const bool pframes = p.video && p.gop > 1;  // I/P-frame video (VideoEncoder.cpp:83-91 with gop)
    const size_t cap = pframes ? ie_gop_stream_bound(p.w, p.h, p.n, p.frames, p.merange, H)
                               : ie_stream_bound(p.w, p.h, p.n, p.frames, H);
    if (!cap) return (err = "invalid dimensions", IE_EINVAL);
    if ((r = s.enc.reserve(cap))) return (err = ie_last_error(c), r);
    const size_t hb = size_t((H + 7) / 8);
    // the P-frame records are ORed into the stream: it must be zero from the header on
    if ((r = ie_memset(c, s.enc.p, 0, pframes ? cap : hb + 4))) return (err = ie_last_error(c), r);
    if ((r = ie_memcpy(c, s.enc.p, hdr.get_buffer(), hb))) return (err = ie_last_error(c), r);
    uint64_t end = 0;
    if (pframes) {  // the groups of pictures side by side: ie_encode_gop's bytes, a launch chain as deep as gop
        if ((r = ie_encode_gop_groups(c, y, p.w, p.h, size_t(p.w), p.frame_pitch, p.frames, p.gop, p.merange,
                                      p.rle ? 1 : 0, p.mode, s.enc.p, s.enc.cap, H, nullptr, &end)))
            return (err = ie_last_error(c), r);
    } else if ((r = ie_encode_frames(c, y, p.w, p.h, size_t(p.w), p.frame_pitch, p.frames, p.rle ? 1 : 0, p.mode,
                                     s.enc.p, s.enc.cap, H, nullptr, &end)))
        return (err = ie_last_error(c), r);
    const size_t bytes = size_t((end + 7) / 8);
    if (pre_bytes) *pre_bytes = bytes;
    if (!p.huffman) {
        out.resize(bytes);
        if ((r = ie_memcpy(c, out.data(), s.enc.p, bytes))) return (err = ie_last_error(c), r);
        return IE_OK;
    }
    const int64_t hl = algo::huffman_device(c, s.enc.p, bytes, s.huf, err);
    if (hl < 0) return int(hl);
    out.resize(size_t(hl));
    if ((r = ie_memcpy(c, out.data(), s.huf.p, size_t(hl)))) return (err = ie_last_error(c), r);
    return IE_OK;
}

// A video file encoded while it is read: frame chunks go from the .raw/YUV420 file into two
// page-locked buffers in turn (VideoBase.cpp:6-19 and utils.hpp:352-376 read the whole file
// first), each chunk is pushed to an ie_vstream -- copied to the device and encoded behind the
// previous chunk on the device's chain (with P-frames, gop > 1: whole groups of pictures side by
// side, ie_vstream_open_gop) -- while the host reads the next one, and the finished bytes are
// pulled out as the chunks complete.  The host holds two read buffers and the device two input
// slots, one wave of scratch and the output stream, never the whole video.  With Huffman the
// stream stays on the device for the Huffman pass over the whole file (Huffman.cpp:233-344 needs
// every byte's count first).
int encode_video_streamed(ie_ctx* c, const std::string& path, const FileParams& p, std::vector<uint8_t>& out,
                          std::string& err) {
    if (!c) return (err = "no GPU context", IE_EHIP);
    int r;
    if ((r = ie_set_quant(c, p.q, p.n))) return (err = ie_last_error(c), r);
    util::BitStreamWriter hdr(64);
    write_header(hdr, p);
    const uint64_t H = hdr.get_position();
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return (err = "Could not read file '" + path + "'", IE_EINVAL);
    ie_vstream* v = nullptr;
    if ((r = ie_vstream_open_gop(c, p.w, p.h, size_t(p.w), p.frame_pitch, p.gop, p.merange, p.rle ? 1 : 0, p.mode,
                                 hdr.get_buffer(), H, p.frames, &v))) {
        std::fclose(f);
        return (err = ie_last_error(c), r);
    }
    // ~32 MiB of frames per read (IE_CHUNK_MB: a tuning aid; the output does not depend on it)
    const char* ce = std::getenv("IE_CHUNK_MB");
    const size_t target = (ce && std::atof(ce) > 0) ? size_t(std::atof(ce) * 1048576.0) : (size_t(32) << 20);
    const int K = int(std::max<size_t>(1, std::min<size_t>(size_t(p.frames), target / p.frame_pitch)));
    uint8_t* buf[2] = {nullptr, nullptr};
    for (int i = 0; i < 2 && r == IE_OK; i++) {
        void* b = nullptr;
        r = ie_host_alloc(c, size_t(K) * p.frame_pitch, &b);
        buf[i] = static_cast<uint8_t*>(b);
    }
    if (!p.huffman)
        out.assign(p.gop > 1 ? ie_gop_stream_bound(p.w, p.h, p.n, p.frames, p.merange, H)
                             : ie_stream_bound(p.w, p.h, p.n, p.frames, H),
                   0);
    size_t got = 0, nb = 0;
    auto read_chunk = [&](int i, int nf) {
        return std::fread(buf[i], p.frame_pitch, size_t(nf), f) == size_t(nf);
    };
    int f0 = 0, slot = 0;
    int nf = std::min(K, p.frames);
    if (r == IE_OK && !read_chunk(0, nf)) r = (err = "short read of '" + path + "'", IE_EINVAL);
    while (r == IE_OK && f0 < p.frames) {
        // the push DMAs from buf[slot] asynchronously; buf[slot^1] was released by this push
        if ((r = ie_vstream_push(v, buf[slot], nf))) break;
        const int f1 = f0 + nf, nf1 = std::min(K, p.frames - f1);
        if (nf1 > 0 && !read_chunk(slot ^ 1, nf1)) {
            r = (err = "short read of '" + path + "'", IE_EINVAL);
            break;
        }
        if (!p.huffman && (r = ie_vstream_pull(v, out.data() + got, out.size() - got, &nb))) break;
        got += nb;
        f0 = f1;
        nf = nf1;
        slot ^= 1;
    }
    uint64_t end = 0;
    if (r == IE_OK)
        r = p.huffman ? ie_vstream_finish(v, nullptr, 0, nullptr, &end, nullptr)
                      : ie_vstream_finish(v, out.data() + got, out.size() - got, &nb, &end, nullptr);
    if (r == IE_OK && !p.huffman) out.resize(got + nb);
    if (r == IE_OK && p.huffman) {
        Scratch& s = scratch(c);
        const int64_t hl = algo::huffman_device(c, ie_vstream_device(v), size_t((end + 7) / 8), s.huf, err);
        if (hl < 0) r = int(hl);
        else {
            out.resize(size_t(hl));
            if ((r = ie_memcpy(c, out.data(), s.huf.p, size_t(hl)))) err = ie_last_error(c);
        }
    } else if (r != IE_OK && err.empty()) {
        err = ie_last_error(c);
    }
    ie_vstream_close(v);
    for (uint8_t* b : buf) ie_host_free(c, b);
    std::fclose(f);
    return r;
}

// Parse a (Huffman-decoded) image or video stream header.  Returns false on a short stream.
struct StreamHeader {
    std::vector<uint16_t> q;
    int rle = 0, w = 0, h = 0, frames = 1, gop = 1, merange = 0;
    uint64_t payload_bit = 0;
};

static bool parse_header(const uint8_t* src, size_t len, size_t start, int n, bool video, StreamHeader& sh) {
    util::BitStreamReader rd(src, len);
    rd.set_position(start);
    if (n == 8) {  // MatrixReader<N>::fromBitstream (MatrixReader.cpp:46-56)
        const MatrixReader<8> m = MatrixReader<8>::fromBitstream(rd);
        sh.q.assign(m.data(), m.data() + 64);
    } else {
        const MatrixReader<4> m = MatrixReader<4>::fromBitstream(rd);
        sh.q.assign(m.data(), m.data() + 16);
    }
    sh.rle = int(rd.get(1));
    sh.w = int(rd.get(15));
    sh.h = int(rd.get(15));
    if (video) {
        sh.frames = int(rd.get(15));
        sh.gop = int(rd.get(15));
        sh.merange = int(rd.get(15));
    }
    sh.payload_bit = rd.get_position();
    return sh.payload_bit <= uint64_t(len) * 8;
}

// Decode a file image into frames of pixels.  out_frame_pitch bytes per decoded frame.
// Video frames come out as Y followed by w*h/2 bytes of UV fill.
// cap: the caller's pixel capacity -- a smaller one returns IE_ECAP right after the header (sh
// filled in), before the payload is decoded
// The front half of every file decode: the Huffman pass (dec: its output when the file has a
// dictionary), the settings header, ie_set_quant.  *src / *srclen: the stream the payload is in.
static int decode_front(ie_ctx* c, const uint8_t* enc, size_t len, int n, bool video, StreamHeader& sh,
                        std::vector<uint8_t>& dec, const uint8_t** src, size_t* srclen, std::string& err) {
    if (!c) return (err = "no GPU context", IE_EHIP);
    bool pass = false;
    size_t start = 0;
    if (int r = algo::Huffman::decode(c, enc, len, dec, pass, start))
        return (err = (r == IE_EFORMAT ? std::string("malformed Huffman stream") : std::string(ie_last_error(c))), r);
    *src = pass ? enc : dec.data();
    *srclen = pass ? len : dec.size();
    if (!parse_header(*src, *srclen, start, n, video, sh)) return (err = "stream shorter than its header", IE_EFORMAT);
    if (int r = ie_set_quant(c, sh.q.data(), n)) return (err = ie_last_error(c), r);
    return IE_OK;
}

static int decode_file(ie_ctx* c, const uint8_t* enc, size_t len, int n, bool video, StreamHeader& sh,
                       std::vector<uint8_t>& pix, std::string& err, size_t cap = SIZE_MAX, bool motioncomp = true) {
    std::vector<uint8_t> dec;
    const uint8_t* src = nullptr;
    size_t srclen = 0;
    int r;
    if ((r = decode_front(c, enc, len, n, video, sh, dec, &src, &srclen, err))) return r;
    const size_t fbytes = size_t(sh.w) * sh.h;
    const size_t pitch = video ? fbytes + fbytes / 2 : fbytes;
    if (pitch * size_t(sh.frames) > cap) return IE_ECAP;
    pix.assign(pitch * size_t(sh.frames), video ? 0x80 : 0);  // UV fill (Frame.cpp:121-124)
    if (!fbytes || !sh.frames) return IE_OK;
    if (video && sh.gop > 1) {  // P-frames: frame by frame (Frame::loadFromStream, Frame.cpp:47-127)
        if ((r = ie_decode_gop(c, src, srclen, sh.payload_bit, sh.w, sh.h, sh.frames, sh.gop, sh.merange, sh.rle,
                               motioncomp ? 1 : 0, pix.data(), size_t(sh.w), pitch, nullptr)))
            return (err = ie_last_error(c), r);
        return IE_OK;
    }
    if ((r = ie_decode_frames(c, src, srclen, sh.payload_bit, sh.w, sh.h, sh.frames, sh.rle, pix.data(), size_t(sh.w),
                              pitch, nullptr)))
        return (err = ie_last_error(c), r);
    return IE_OK;
}

}  // namespace dc

// A video file decoded chunk by chunk (ieh_vdec_*): decode_file's front half, then an ie_vdec over
// the payload.  The Huffman-decoded stream (if any) is the decoder's own copy on the device, so
// nothing of the file is kept on the host after open.
struct ieh_vdec {
    ie_ctx* c = nullptr;
    ie_vdec* v = nullptr;
    dc::StreamHeader sh;
    size_t done = 0;  // frames handed out
};

namespace dc {

static int vdec_open(ie_ctx* c, const uint8_t* enc, size_t len, int n, bool motioncomp, int chunk_frames,
                     ieh_vdec** out, std::string& err) {
    std::unique_ptr<ieh_vdec> d(new ieh_vdec());
    d->c = c;
    std::vector<uint8_t> dec;
    const uint8_t* src = nullptr;
    size_t srclen = 0;
    int r;
    if ((r = decode_front(c, enc, len, n, true, d->sh, dec, &src, &srclen, err))) return r;
    const StreamHeader& sh = d->sh;
    if (sh.w && sh.h && sh.frames &&
        (r = ie_vdec_open(c, src, srclen, sh.payload_bit, sh.w, sh.h, sh.frames, sh.gop, sh.merange, sh.rle,
                          motioncomp ? 1 : 0, chunk_frames, &d->v)))
        return (err = ie_last_error(c), r);
    *out = d.release();
    return IE_OK;
}

// Whole frames in the file's layout -- Y, then w*h/2 bytes of 0x80 (Frame.cpp:121-124) -- as many as
// cap holds.  An error leaves *got at the frames written before it.
static int vdec_next(ieh_vdec* d, uint8_t* out, size_t cap, int* got, std::string& err) {
    *got = 0;
    const size_t fbytes = size_t(d->sh.w) * d->sh.h, pitch = fbytes + fbytes / 2;
    if (!d->v || !pitch) return IE_OK;
    const size_t room = std::min<size_t>(cap / pitch, size_t(d->sh.frames) - d->done);
    if (!room) return IE_OK;
    const int r = ie_vdec_next(d->v, out, size_t(d->sh.w), pitch, int(std::min<size_t>(room, size_t(INT32_MAX))), got);
    for (int i = 0; i < *got; i++) std::memset(out + size_t(i) * pitch + fbytes, 0x80, pitch - fbytes);
    d->done += size_t(*got);
    if (r) err = ie_last_error(d->c);
    return r;
}

static void vdec_close(ieh_vdec* d) {
    if (!d) return;
    ie_vdec_close(d->v);
    delete d;
}

// A batch of image files with the same settings into pixels, w*h bytes per image back to back in
// file order (ieh_decode_images).  The decoded streams never leave the device: the dictionaries are
// parsed on the host, ONE ie_huffman_decode_batch call decodes every coded file into device slots
// and brings back the symbol counts with the first kHeadBytes bytes of every slot (the settings
// headers) in its one synchronisation, and ONE ie_decode_images call reads the slots in place --
// two synchronisations for a batch of coded files.  Files without a dictionary (the "no gain"
// output of Huffman.cpp:329-341) form a second group that ie_decode_images reads straight from
// the file bytes.  A group whose files are not adjacent in the batch is decoded into device
// scratch and its images copied to their places.
constexpr size_t kHeadBytes = 256;  // (an 8x8 header is at most 5 + 64*16 + 1 + 30 bits)

static int64_t decode_files(ie_ctx* c, const uint8_t* enc, size_t enc_pitch, const uint64_t* len, int count, int n,
                            uint8_t* out, size_t cap, int* w, int* h) {
    auto failk = [&](int code, int k, const std::string& what) {
        ie_set_error(c, ("file " + std::to_string(k) + ": " + what).c_str());
        return int64_t(code);
    };
    const size_t K = size_t(count);
    struct Group {
        std::vector<int> file;        // the group's files, in file order
        std::vector<uint64_t> start;  // coded: the code stream's first bit; else the header's
        std::vector<uint64_t> bytes;
    } coded, plain;
    std::vector<int> at(K);  // a file's place in its group
    std::vector<char> is_plain(K, 0);
    std::vector<uint16_t> luts, lut(size_t(1) << 15);
    for (int k = 0; k < count; k++) {
        if (len[k] > enc_pitch) return failk(IE_EINVAL, k, "len beyond its slot of enc_pitch bytes");
        uint64_t from = 0;
        const int r = ie_huffman_table(enc + size_t(k) * enc_pitch, size_t(len[k]), 0, lut.data(), &from);
        if (r < 0) return failk(r, k, "malformed Huffman dictionary");
        Group& g = r == 1 ? plain : coded;
        is_plain[size_t(k)] = r == 1;
        at[size_t(k)] = int(g.file.size());
        g.file.push_back(k);
        g.start.push_back(from);
        g.bytes.push_back(len[k]);
        if (r == 0) luts.insert(luts.end(), lut.begin(), lut.end());
    }
    // a group's files as one pitched array: the caller's when the group is the whole batch
    std::vector<uint8_t> gathered[2];
    auto pitched = [&](const Group& g, std::vector<uint8_t>& buf, size_t* pitch) -> const uint8_t* {
        if (g.file.size() == K) return (*pitch = enc_pitch, enc);
        uint64_t longest = 0;
        for (uint64_t b : g.bytes) longest = std::max(longest, b);
        *pitch = std::max<size_t>((size_t(longest) + 15) / 16 * 16, 16);
        buf.assign(*pitch * g.file.size(), 0);
        for (size_t j = 0; j < g.file.size(); j++)
            std::memcpy(&buf[j * *pitch], enc + size_t(g.file[j]) * enc_pitch, size_t(g.bytes[j]));
        return buf.data();
    };
    Scratch& s = scratch(c);
    int r;
    size_t slot_pitch = 0;
    std::vector<uint64_t> nout(coded.file.size());
    std::vector<uint8_t> heads(coded.file.size() * kHeadBytes);
    if (!coded.file.empty()) {
        size_t pitch = 0;
        const uint8_t* in = pitched(coded, gathered[0], &pitch);
        r = algo::huffman_decode_device_batch(c, in, pitch, coded.bytes.data(), int(coded.file.size()), coded.start.data(),
                                              luts.data(), s.huf, &slot_pitch, nout.data(), heads.data(), kHeadBytes);
        if (r == IE_EFORMAT)
            for (size_t j = 0; j < nout.size(); j++)
                if (nout[j] == UINT64_MAX) return failk(r, coded.file[j], "malformed Huffman stream");
        if (r) return r;
    }
    std::vector<StreamHeader> sh(K);
    for (int k = 0; k < count; k++) {
        const size_t j = size_t(at[size_t(k)]);
        const bool ok = is_plain[size_t(k)]
                            ? parse_header(enc + size_t(k) * enc_pitch, size_t(len[k]), size_t(plain.start[j]), n, false, sh[size_t(k)])
                            : parse_header(&heads[j * kHeadBytes], size_t(std::min<uint64_t>(nout[j], kHeadBytes)), 0, n, false,
                                           sh[size_t(k)]);
        if (!ok) return failk(IE_EFORMAT, k, "stream shorter than its header");
        const StreamHeader &a = sh[0], &b = sh[size_t(k)];
        const StreamHeader& g0 = sh[size_t((is_plain[size_t(k)] ? plain : coded).file[0])];
        if (a.q != b.q || a.rle != b.rle || a.w != b.w || a.h != b.h || g0.payload_bit != b.payload_bit)
            return failk(IE_EINVAL, k, "settings differ from file 0's (one quant matrix, rle, width and height per batch)");
    }
    if (w) *w = sh[0].w;
    if (h) *h = sh[0].h;
    const size_t fbytes = size_t(sh[0].w) * sh[0].h;
    if (fbytes * K > cap) return (ie_set_error(c, "pixel capacity below count * w * h"), IE_ECAP);
    if (!fbytes) return 0;
    if ((r = ie_set_quant(c, sh[0].q.data(), n))) return r;
    auto decode_group = [&](const Group& g, const uint8_t* in, size_t pitch, const std::vector<uint64_t>& nbits) -> int64_t {
        const size_t m = g.file.size();
        const bool adjacent = size_t(g.file.back() - g.file.front()) + 1 == m;
        int rr;
        if (!adjacent && (rr = s.pix.reserve(m * fbytes))) return rr;
        uint8_t* dst = adjacent ? out + size_t(g.file.front()) * fbytes : s.pix.p;
        std::vector<uint64_t> ends(m);
        const StreamHeader& g0 = sh[size_t(g.file[0])];
        rr = ie_decode_images(c, in, pitch, nbits.data(), int(m), g0.payload_bit, g0.w, g0.h, g0.rle, dst, size_t(g0.w),
                              fbytes, ends.data());
        if (rr == IE_EFORMAT)
            for (size_t j = 0; j < m; j++)
                if (ends[j] == UINT64_MAX) return failk(rr, g.file[j], "stream ends before the last block");
        if (rr) return rr;
        for (size_t j = 0; !adjacent && j < m; j++)
            if ((rr = ie_memcpy(c, out + size_t(g.file[j]) * fbytes, s.pix.p + j * fbytes, fbytes))) return rr;
        return IE_OK;
    };
    if (!coded.file.empty()) {
        std::vector<uint64_t> nbits(nout.size());
        for (size_t j = 0; j < nout.size(); j++) nbits[j] = 8 * nout[j];
        if (int64_t e = decode_group(coded, s.huf.p, slot_pitch, nbits)) return e;
    }
    if (!plain.file.empty()) {
        size_t pitch = 0;
        const uint8_t* in = pitched(plain, gathered[1], &pitch);
        std::vector<uint64_t> nbits(plain.bytes.size());
        for (size_t j = 0; j < nbits.size(); j++) nbits[j] = 8 * plain.bytes[j];
        if (int64_t e = decode_group(plain, in, pitch, nbits)) return e;
    }
    return int64_t(fbytes * K);
}

// ----------------------------------------------------------------------------- ImageProcessor
ImageProcessor::ImageProcessor(const std::string& src, const std::string& dst, uint16_t w, uint16_t h, bool rle,
                               QuantSpec quant)
    : width(w), height(h), use_rle(rle), quant_m(std::move(quant)), source_file(src), dest_file(dst) {
    if (!read_file(source_file, raw)) err_ = "Could not read file '" + source_file + "'";
}

ImageProcessor::ImageProcessor(const std::string& src, const std::string& dst) : source_file(src), dest_file(dst) {
    if (!read_file(source_file, raw)) err_ = "Could not read file '" + source_file + "'";
}

void ImageProcessor::saveResult(bool encoded) const {
    if (!write_file(dest_file, result_)) util::Logger::WriteLn("[ImageProcessor] Could not write '" + dest_file + "'");
    if (encoded) {
        util::Logger::WriteLn(fmt("[ImageProcessor] Original file size: %8.0f bytes", double(raw.size())));
        util::Logger::WriteLn(fmt("[ImageProcessor]        Encoded size: %8.0f bytes  => Ratio: %.2f%%",
                                  double(result_.size()),
                                  raw.empty() ? 0.0 : 100.0 * double(result_.size()) / double(raw.size())));
    }
    util::Logger::WriteLn("[ImageProcessor] Saved file at: " + dest_file);
}

// ------------------------------------------------------------------------------- ImageEncoder
bool ImageEncoder::process() {
    if (!err_.empty()) return false;
    util::Logger::WriteLn("[ImageEncoder] Processing image...");
    const int n = quant_m.n;
    if (width % n || height % n) return (err_ = "width and height must be multiples of the block size", false);
    if (raw.size() != size_t(width) * height) return (err_ = "raw file size differs from width x height", false);
    const FileParams p = image_params(width, height, n, quant_m.q.data(), use_rle, opt_.huffman, opt_.mode);
    return encode_file(Device::get(), raw.data(), p, result_, err_) == IE_OK;
}

// ------------------------------------------------------------------------------- ImageDecoder
ImageDecoder::ImageDecoder(const std::string& source_file, const std::string& dest_file, int block_size)
    : ImageProcessor(source_file, dest_file), n_(block_size ? block_size : block_size_from_env()) {}

bool ImageDecoder::process() {
    if (!err_.empty()) return false;
    util::Logger::WriteLn("[ImageDecoder] Processing image...");
    StreamHeader sh;
    if (decode_file(Device::get(), raw.data(), raw.size(), n_, false, sh, result_, err_) != IE_OK) return false;
    width = uint16_t(sh.w);
    height = uint16_t(sh.h);
    use_rle = sh.rle != 0;
    quant_m.n = n_;
    quant_m.q = sh.q;
    return true;
}

// ----------------------------------------------------------------------------- VideoProcessor
VideoProcessor::VideoProcessor(const std::string& src, const std::string& dst, uint16_t w, uint16_t h, bool rle,
                               QuantSpec quant, uint16_t g, uint16_t mer)
    : width(w), height(h), gop(g ? g : 1), merange(mer), use_rle(rle), quant_m(std::move(quant)), source_file(src),
      dest_file(dst) {
    // (VideoBase.cpp:6-19 reads the whole file here; the encoder streams it in process())
    std::ifstream f(source_file, std::ios::binary | std::ios::ate);
    if (!f) err_ = "Could not read file '" + source_file + "'";
    else raw_size = size_t(f.tellg());
}

VideoProcessor::VideoProcessor(const std::string& src, const std::string& dst, const bool& mc)
    : motioncomp(mc), source_file(src), dest_file(dst) {
    if (!read_file(source_file, raw)) err_ = "Could not read file '" + source_file + "'";
    raw_size = raw.size();
}

void VideoProcessor::saveResult(bool encoded) const {
    if (!write_file(dest_file, result_)) util::Logger::WriteLn("[VideoProcessor] Could not write '" + dest_file + "'");
    if (encoded) {
        util::Logger::WriteLn(fmt("[VideoProcessor] Original file size: %8.0f bytes", double(raw_size)));
        util::Logger::WriteLn(fmt("[VideoProcessor]       Encoded size: %8.0f bytes  => Ratio: %.2f%%",
                                  double(result_.size()),
                                  raw_size ? 100.0 * double(result_.size()) / double(raw_size) : 0.0));
    }
    util::Logger::WriteLn("[VideoProcessor] Saved file at: " + dest_file);
}

// ------------------------------------------------------------------------------- VideoEncoder
bool VideoEncoder::process() {
    if (!err_.empty()) return false;
    util::Logger::WriteLn("[VideoEncoder] Processing video...");
    const int n = quant_m.n;
    if (width % n || height % n) return (err_ = "width and height must be multiples of the block size", false);
    FileParams p;
    if (!video_params(width, height, n, quant_m.q.data(), use_rle, opt_.huffman, opt_.mode, raw_size, gop, merange, &p))
        return (err_ = "frame count must be in 1..32767", false);
    return encode_video_streamed(Device::get(), source_file, p, result_, err_) == IE_OK;
}

// ------------------------------------------------------------------------------- VideoDecoder
VideoDecoder::VideoDecoder(const std::string& source_file, const std::string& dest_file, const bool& mc,
                           int block_size, bool stream_to_file)
    : VideoProcessor(source_file, dest_file, mc), n_(block_size ? block_size : block_size_from_env()),
      stream_to_file_(stream_to_file) {}

// The frames written to dest_file as their chunks arrive: two page-locked buffers of a chunk of
// frames in turn, so the write of one chunk runs while the next one crosses.  A failure removes the
// partial file: a failed run leaves no output, as before.
bool VideoDecoder::processToFile() {
    ie_ctx* c = Device::get();
    ieh_vdec* d = nullptr;
    if (vdec_open(c, raw.data(), raw.size(), n_, motioncomp, 0, &d, err_) != IE_OK) return false;
    const StreamHeader sh = d->sh;
    std::vector<uint8_t>().swap(raw);  // (the decoder has its own copy of the stream)
    const size_t fbytes = size_t(sh.w) * sh.h, pitch = fbytes + fbytes / 2;
    int K = 1;
    if (d->v) ie_vdec_info(d->v, &K, nullptr, nullptr, nullptr);
    K = std::max(1, std::min(K, sh.frames));
    FILE* f = std::fopen(dest_file.c_str(), "wb");
    bool ok = f != nullptr;
    if (!ok) err_ = "Could not write '" + dest_file + "'";
    void* buf = nullptr;
    if (ok && pitch && ie_host_alloc(c, size_t(K) * pitch, &buf) != IE_OK) ok = (err_ = ie_last_error(c), false);
    size_t frames = 0;
    while (ok && frames < size_t(sh.frames) && pitch) {
        int got = 0;
        if (vdec_next(d, static_cast<uint8_t*>(buf), size_t(K) * pitch, &got, err_) != IE_OK || got == 0) {
            if (err_.empty()) err_ = "stream ends before the last block";
            ok = false;
        } else if (std::fwrite(buf, pitch, size_t(got), f) != size_t(got)) {
            ok = (err_ = "Could not write '" + dest_file + "'", false);
        }
        frames += size_t(got);
    }
    if (buf) ie_host_free(c, buf);
    vdec_close(d);
    if (f && std::fclose(f) != 0 && ok) ok = (err_ = "Could not write '" + dest_file + "'", false);
    if (!ok && f) std::remove(dest_file.c_str());
    if (!ok) return false;
    width = uint16_t(sh.w);
    height = uint16_t(sh.h);
    gop = uint16_t(sh.gop);
    merange = uint16_t(sh.merange);
    return true;
}

void VideoDecoder::saveResult() const {
    if (!stream_to_file_) return VideoProcessor::saveResult(false);
    util::Logger::WriteLn("[VideoProcessor] Saved file at: " + dest_file);  // (process() wrote it)
}

bool VideoDecoder::process() {
    if (!err_.empty()) return false;
    util::Logger::WriteLn("[VideoDecoder] Processing video...");
    if (stream_to_file_) return processToFile();
    StreamHeader sh;
    if (decode_file(Device::get(), raw.data(), raw.size(), n_, true, sh, result_, err_, SIZE_MAX, motioncomp) != IE_OK)
        return false;
    width = uint16_t(sh.w);
    height = uint16_t(sh.h);
    gop = uint16_t(sh.gop);
    merange = uint16_t(sh.merange);
    return true;
}

}  // namespace dc

// ---------------------------------------------------------------------------------- C entry
extern "C" {

int64_t ieh_write_header(uint8_t* out, size_t cap, int n, const uint16_t* q, int rle, int w, int h, int huffman,
                         int video, int frames, int gop, int merange) {
    if (!out || !q || (n != 4 && n != 8)) return IE_EINVAL;
    dc::FileParams p = dc::image_params(w, h, n, q, rle != 0, huffman != 0, IE_MODE_FAST);
    p.video = video != 0;
    p.frames = frames;
    p.gop = gop;
    p.merange = merange;
    util::BitStreamWriter hdr(64);
    dc::write_header(hdr, p);
    const size_t bytes = hdr.get_last_byte_position();
    if (bytes > cap) return IE_ECAP;
    std::memset(out, 0, cap);
    std::memcpy(out, hdr.get_buffer(), bytes);
    return int64_t(hdr.get_position());
}

int64_t ieh_encode_image(ie_ctx* c, const uint8_t* y, int w, int h, const uint16_t* q, int n, int rle, int huffman,
                         int mode, uint8_t* out, size_t cap) {
    if (!c || !y || !q || !out) return IE_EINVAL;
    const dc::FileParams p = dc::image_params(w, h, n, q, rle != 0, huffman != 0, mode);
    std::vector<uint8_t> v;
    std::string err;
    const int r = dc::encode_file(c, y, p, v, err);
    if (r) return r;
    if (v.size() > cap) return IE_ECAP;
    std::memcpy(out, v.data(), v.size());
    return int64_t(v.size());
}

// ---- rate control: scale the matrix until the file fits a byte budget (ie_probe_sizes) or until
// its distortion meets a target (ie_probe_rd)
namespace {
// round(100 * 2^(j/4)), j = -8 .. 23: the scales the budget search probes first
const int kBudgetLadder[32] = {25,  30,  35,  42,  50,  59,  71,   84,   100,  119,  141,  168,  200,  238,  283,  336,
                               400, 476, 566, 673, 800, 951, 1131, 1345, 1600, 1903, 2263, 2691, 3200, 3805, 4525, 5382};

// File bytes (before any Huffman pass) of every percent in `pc` for one frame, and with `sse` the
// squared error of the decoded frame: one ie_probe_sizes / ie_probe_rd call over the distinct
// scaled matrices, mapped back to the percents.  A video file (p.video; sizes only): one
// ie_probe_gop call over its frames' Y planes, the frames' bits summed; with `sse` one ie_probe_gop_rd
// call judged for the decoder setting `motioncomp`, the frames' errors summed and, with `frame_sse`,
// kept per percent as well ([pc.size()][p.frames]).
int probe_percents(ie_ctx* c, const uint8_t* y, dc::FileParams p, const uint16_t* base, const std::vector<int>& pc,
                   std::vector<uint64_t>& bytes, std::vector<uint64_t>* sse = nullptr, int motioncomp = 1,
                   std::vector<uint64_t>* frame_sse = nullptr) {
    const int nn = p.n * p.n;
    std::vector<uint16_t> qs;        // the distinct matrices, in order of first use
    std::vector<int> which(pc.size());
    std::vector<uint16_t> q(static_cast<size_t>(nn));
    for (size_t i = 0; i < pc.size(); i++) {
        ieh_scale_matrix(base, p.n, pc[i], q.data());
        size_t m = 0;
        for (; m * nn < qs.size(); m++)
            if (std::equal(q.begin(), q.end(), qs.begin() + m * nn)) break;
        if (m * nn == qs.size()) qs.insert(qs.end(), q.begin(), q.end());
        which[i] = int(m);
    }
    const int nq = int(qs.size() / size_t(nn));
    std::vector<uint64_t> bits(static_cast<size_t>(nq), 0), se(static_cast<size_t>(nq), 0);
    int r;
    std::vector<uint64_t> fse;  // a video's squared errors per matrix and frame
    if (p.video) {
        std::vector<uint64_t> fbits(static_cast<size_t>(nq) * size_t(p.frames), 0);
        if (sse) {
            fse.assign(fbits.size(), 0);
            r = ie_probe_gop_rd(c, y, p.w, p.h, size_t(p.w), p.frame_pitch, p.frames, p.gop, p.merange, p.rle ? 1 : 0,
                                motioncomp, qs.data(), nq, fbits.data(), fse.data());
        } else {
            r = ie_probe_gop(c, y, p.w, p.h, size_t(p.w), p.frame_pitch, p.frames, p.gop, p.merange, p.rle ? 1 : 0,
                             qs.data(), nq, fbits.data());
        }
        for (int m = 0; m < nq; m++) {
            bits[size_t(m)] = std::accumulate(fbits.begin() + size_t(m) * p.frames, fbits.begin() + size_t(m + 1) * p.frames,
                                              uint64_t(0));
            if (sse)
                se[size_t(m)] = std::accumulate(fse.begin() + size_t(m) * p.frames, fse.begin() + size_t(m + 1) * p.frames,
                                                uint64_t(0));
        }
    } else {
        r = sse ? ie_probe_rd(c, y, p.w, p.h, size_t(p.w), 0, 1, p.rle ? 1 : 0, qs.data(), nq, bits.data(), se.data())
                : ie_probe_sizes(c, y, p.w, p.h, size_t(p.w), 0, 1, p.rle ? 1 : 0, qs.data(), nq, bits.data());
    }
    if (r) return r;
    bytes.resize(pc.size());
    if (sse) sse->resize(pc.size());
    if (frame_sse) frame_sse->resize(pc.size() * size_t(p.frames));
    for (size_t i = 0; i < pc.size(); i++) {
        if (frame_sse)
            std::copy(fse.begin() + size_t(which[i]) * p.frames, fse.begin() + size_t(which[i] + 1) * p.frames,
                      frame_sse->begin() + i * size_t(p.frames));
        p.q = qs.data() + size_t(which[i]) * nn;
        util::BitStreamWriter hdr(64);
        dc::write_header(hdr, p);  // (its length depends on the matrix's widest value)
        bytes[i] = (uint64_t(hdr.get_position()) + bits[size_t(which[i])] + 7) / 8;
        if (sse) (*sse)[i] = se[size_t(which[i])];
    }
    return IE_OK;
}

// The integers p0 + ceil(i (p1 - p0) / 33), i = 1 .. 32, strictly between two ladder entries: at
// most 32 of them, ascending.
std::vector<int> refine_percents(int p0, int p1) {
    std::vector<int> fine;
    for (int i = 1; i <= 32; i++) {
        const int v = p0 + (i * (p1 - p0) + 32) / 33;
        if (v > p0 && v < p1 && (fine.empty() || fine.back() != v)) fine.push_back(v);
    }
    return fine;
}

// Host frames (px bytes) go to the device once, for the probes and the encode.
int frames_on_device(ie_ctx* c, const uint8_t* y, size_t px, const uint8_t** dy) {
    *dy = y;
    if (!dc::is_device(c, y) && px > 0) {
        dc::Scratch& s = dc::scratch(c);
        int r;
        if ((r = s.pix.reserve(px))) return r;
        if ((r = ie_memcpy(c, s.pix.p, y, px))) return r;
        *dy = s.pix.p;
    }
    return IE_OK;
}
int frame_on_device(ie_ctx* c, const uint8_t* y, int w, int h, const uint8_t** dy) {
    return frames_on_device(c, y, w > 0 && h > 0 ? size_t(w) * size_t(h) : 0, dy);
}

// The file under `base` scaled to `percent`, which the probe sized at probed_bytes before the Huffman pass.
int64_t encode_scaled(ie_ctx* c, const uint8_t* dy, dc::FileParams p, const uint16_t* base, int percent,
                      uint64_t probed_bytes, const char* what, uint8_t* out, size_t cap, int* chosen) {
    std::vector<uint16_t> q(static_cast<size_t>(p.n * p.n));
    ieh_scale_matrix(base, p.n, percent, q.data());
    p.q = q.data();
    std::vector<uint8_t> v;
    std::string err;
    size_t pre = 0;
    int r;
    if ((r = dc::encode_file(c, dy, p, v, err, &pre))) return r;
    *chosen = percent;
    if (uint64_t(pre) != probed_bytes) {
        ie_set_error(c, (std::string(what) + " encode: the file is " + std::to_string(pre) +
                         " bytes before the Huffman pass, the probe said " + std::to_string(probed_bytes)).c_str());
        return IE_EDEVICE;
    }
    if (v.size() > cap) {
        ie_set_error(c, "output capacity below the encoded file");
        return IE_ECAP;
    }
    std::memcpy(out, v.data(), v.size());
    return int64_t(v.size());
}

// The budget search over device frames dy (an image, or a video's YUV420 frames: p.video): the
// ladder, the refinement between its two entries, the encode of the smallest percent that fits.
int64_t encode_budget(ie_ctx* c, const uint8_t* dy, const dc::FileParams& p, const uint16_t* base, size_t budget_bytes,
                      uint8_t* out, size_t cap, int* percent) {
    int r;
    std::vector<int> ladder(kBudgetLadder, kBudgetLadder + 32);
    std::vector<uint64_t> size;
    if ((r = probe_percents(c, dy, p, base, ladder, size))) return r;
    int i1 = -1;  // the smallest ladder percent whose file fits
    for (int i = 0; i < 32 && i1 < 0; i++)
        if (size[size_t(i)] <= budget_bytes) i1 = i;
    if (i1 < 0) {
        *percent = kBudgetLadder[31];
        ie_set_error(c, "no scale up to 5382 % meets the budget");
        return IE_ECAP;
    }
    int best = kBudgetLadder[i1];
    uint64_t best_bytes = size[size_t(i1)];
    if (i1 > 0) {  // the integers between the two ladder entries, at most 32 of them
        const std::vector<int> fine = refine_percents(kBudgetLadder[i1 - 1], kBudgetLadder[i1]);
        if (!fine.empty()) {
            std::vector<uint64_t> fsize;
            if ((r = probe_percents(c, dy, p, base, fine, fsize))) return r;
            for (size_t i = 0; i < fine.size(); i++)
                if (fsize[i] <= budget_bytes) {
                    best = fine[i];
                    best_bytes = fsize[i];
                    break;
                }
        }
    }
    return encode_scaled(c, dy, p, base, best, best_bytes, "budget", out, cap, percent);
}

// The quality search over device frames dy (an image, or a video's YUV420 frames: p.video, judged
// for the decoder setting `motioncomp`): the ladder, the refinement above the entry found, the encode
// of the largest percent whose squared error is at most max_sse.  frame_sse (videos, optional):
// the chosen percent's error of every frame.
int64_t encode_quality(ie_ctx* c, const uint8_t* dy, const dc::FileParams& p, const uint16_t* base, uint64_t max_sse,
                       int motioncomp, uint8_t* out, size_t cap, int* percent, uint64_t* sse, uint64_t* frame_sse) {
    int r;
    const size_t nf = size_t(p.frames);
    std::vector<int> ladder(kBudgetLadder, kBudgetLadder + 32);
    std::vector<uint64_t> size, se, fr;
    std::vector<uint64_t>* const pfr = frame_sse ? &fr : nullptr;
    if ((r = probe_percents(c, dy, p, base, ladder, size, &se, motioncomp, pfr))) return r;
    int i0 = -1;  // the largest ladder percent whose distortion meets the target
    for (int i = 0; i < 32; i++)
        if (se[size_t(i)] <= max_sse) i0 = i;
    if (i0 < 0) {
        *percent = kBudgetLadder[0];
        ie_set_error(c, "no scale down to 25 % meets the quality");
        return IE_ECAP;
    }
    int best = kBudgetLadder[i0];
    uint64_t best_bytes = size[size_t(i0)], best_se = se[size_t(i0)];
    if (frame_sse) std::copy(fr.begin() + size_t(i0) * nf, fr.begin() + size_t(i0 + 1) * nf, frame_sse);
    if (i0 < 31) {  // the integers between it and the entry above, at most 32 of them
        const std::vector<int> fine = refine_percents(kBudgetLadder[i0], kBudgetLadder[i0 + 1]);
        if (!fine.empty()) {
            std::vector<uint64_t> fsize, fse;
            if ((r = probe_percents(c, dy, p, base, fine, fsize, &fse, motioncomp, pfr))) return r;
            for (size_t i = 0; i < fine.size(); i++)  // (ascending: the last that meets it is the largest)
                if (fse[i] <= max_sse) {
                    best = fine[i];
                    best_bytes = fsize[i];
                    best_se = fse[i];
                    if (frame_sse) std::copy(fr.begin() + i * nf, fr.begin() + (i + 1) * nf, frame_sse);
                }
        }
    }
    *sse = best_se;
    return encode_scaled(c, dy, p, base, best, best_bytes, "quality", out, cap, percent);
}
}  // namespace

int ieh_budget_ladder(int* out) {
    if (out) std::copy(kBudgetLadder, kBudgetLadder + 32, out);
    return 32;
}

int ieh_scale_matrix(const uint16_t* base, int n, int percent, uint16_t* out) {
    if (!base || !out || (n != 4 && n != 8) || percent < 1) return IE_EINVAL;
    for (int k = 0; k < n * n; k++) {
        const int64_t v = (int64_t(base[k]) * int64_t(percent) + 50) / 100;
        out[k] = uint16_t(std::min<int64_t>(std::max<int64_t>(v, 1), 65535));
    }
    return IE_OK;
}

int64_t ieh_encode_image_budget(ie_ctx* c, const uint8_t* y, int w, int h, const uint16_t* base, int n, int rle,
                                int huffman, int mode, size_t budget_bytes, uint8_t* out, size_t cap, int* percent) {
    if (!c || !y || !base || !out || !percent || (n != 4 && n != 8)) return IE_EINVAL;
    int r;
    if ((r = ie_set_quant(c, base, n))) return r;  // the probe's block size and transform tables
    const dc::FileParams p = dc::image_params(w, h, n, nullptr, rle != 0, huffman != 0, mode);
    const uint8_t* dy;
    if ((r = frame_on_device(c, y, w, h, &dy))) return r;
    return encode_budget(c, dy, p, base, budget_bytes, out, cap, percent);
}

int64_t ieh_encode_image_quality(ie_ctx* c, const uint8_t* y, int w, int h, const uint16_t* base, int n, int rle,
                                 int huffman, int mode, uint64_t max_sse, uint8_t* out, size_t cap, int* percent,
                                 uint64_t* sse) {
    if (!c || !y || !base || !out || !percent || !sse || (n != 4 && n != 8)) return IE_EINVAL;
    int r;
    if ((r = ie_set_quant(c, base, n))) return r;  // the probe's block size and transform tables
    const dc::FileParams p = dc::image_params(w, h, n, nullptr, rle != 0, huffman != 0, mode);
    const uint8_t* dy;
    if ((r = frame_on_device(c, y, w, h, &dy))) return r;
    return encode_quality(c, dy, p, base, max_sse, 1, out, cap, percent, sse, nullptr);
}

int64_t ieh_encode_video(ie_ctx* c, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* q, int n, int rle,
                         int huffman, int merange, int mode, uint8_t* out, size_t cap) {
    return ieh_encode_video_gop(c, yuv, len, w, h, q, n, rle, huffman, 1, merange, mode, out, cap);
}

int64_t ieh_encode_video_gop(ie_ctx* c, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* q, int n,
                             int rle, int huffman, int gop, int merange, int mode, uint8_t* out, size_t cap) {
    if (!c || !yuv || !q || !out || w <= 0 || h <= 0) return IE_EINVAL;
    dc::FileParams p;
    if (!dc::video_params(w, h, n, q, rle != 0, huffman != 0, mode, len, gop, merange, &p)) return IE_EINVAL;
    std::vector<uint8_t> v;
    std::string err;
    const int r = dc::encode_file(c, yuv, p, v, err);
    if (r) return r;
    if (v.size() > cap) return IE_ECAP;
    std::memcpy(out, v.data(), v.size());
    return int64_t(v.size());
}

int64_t ieh_encode_video_budget(ie_ctx* c, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* base, int n,
                                int rle, int huffman, int gop, int merange, int mode, size_t budget_bytes, uint8_t* out,
                                size_t cap, int* percent) {
    if (!c || !yuv || !base || !out || !percent || (n != 4 && n != 8) || w <= 0 || h <= 0) return IE_EINVAL;
    dc::FileParams p;
    if (!dc::video_params(w, h, n, nullptr, rle != 0, huffman != 0, mode, len, gop, merange, &p)) return IE_EINVAL;
    int r;
    if ((r = ie_set_quant(c, base, n))) return r;  // the probe's block size and transform tables
    const uint8_t* dy;
    if ((r = frames_on_device(c, yuv, size_t(p.frames) * p.frame_pitch, &dy))) return r;
    return encode_budget(c, dy, p, base, budget_bytes, out, cap, percent);
}

int64_t ieh_encode_video_quality(ie_ctx* c, const uint8_t* yuv, size_t len, int w, int h, const uint16_t* base, int n,
                                 int rle, int huffman, int gop, int merange, int motioncomp, int mode, uint64_t max_sse,
                                 uint8_t* out, size_t cap, int* percent, uint64_t* sse, uint64_t* frame_sse) {
    if (!c || !yuv || !base || !out || !percent || !sse || (n != 4 && n != 8) || w <= 0 || h <= 0) return IE_EINVAL;
    dc::FileParams p;
    if (!dc::video_params(w, h, n, nullptr, rle != 0, huffman != 0, mode, len, gop, merange, &p)) return IE_EINVAL;
    int r;
    if ((r = ie_set_quant(c, base, n))) return r;  // the probe's block size and transform tables
    const uint8_t* dy;
    if ((r = frames_on_device(c, yuv, size_t(p.frames) * p.frame_pitch, &dy))) return r;
    return encode_quality(c, dy, p, base, max_sse, motioncomp, out, cap, percent, sse, frame_sse);
}

int64_t ieh_decode_image(ie_ctx* c, const uint8_t* enc, size_t len, int n, uint8_t* out, size_t cap, int* w, int* h) {
    if (!c || !enc || !out) return IE_EINVAL;
    dc::StreamHeader sh;
    std::vector<uint8_t> pix;
    std::string err;
    const int r = dc::decode_file(c, enc, len, n, false, sh, pix, err, cap);
    if (w) *w = sh.w;
    if (h) *h = sh.h;
    if (r) return r;
    std::memcpy(out, pix.data(), pix.size());
    return int64_t(pix.size());
}

int64_t ieh_decode_image_region(ie_ctx* c, const uint8_t* enc, size_t len, int n, int x0, int y0, int rw, int rh,
                                uint8_t* out, size_t cap, int* w, int* h) {
    if (!c || !enc || !out) return IE_EINVAL;
    dc::StreamHeader sh;
    std::vector<uint8_t> dec;
    std::string err;
    const uint8_t* src = nullptr;
    size_t srclen = 0;
    int r = dc::decode_front(c, enc, len, n, false, sh, dec, &src, &srclen, err);
    if (w) *w = sh.w;
    if (h) *h = sh.h;
    if (r) return r;
    if (x0 < 0 || y0 < 0 || rw < 1 || rh < 1 || int64_t(x0) + rw > sh.w || int64_t(y0) + rh > sh.h)
        return (ie_set_error(c, "ieh_decode_image_region: the rectangle does not fit the image"), IE_EINVAL);
    const size_t need = size_t(rw) * size_t(rh);
    if (need > cap) return IE_ECAP;
    if ((r = ie_decode_region(c, src, srclen, sh.payload_bit, sh.w, sh.h, 1, sh.rle, x0, y0, rw, rh, out, size_t(rw), need,
                              nullptr)))
        return r;
    return int64_t(need);
}

int64_t ieh_decode_image_scaled(ie_ctx* c, const uint8_t* enc, size_t len, int n, int scale, uint8_t* out, size_t cap, int* w,
                                int* h) {
    if (!c || !enc || !out) return IE_EINVAL;
    dc::StreamHeader sh;
    std::vector<uint8_t> dec;
    std::string err;
    const uint8_t* src = nullptr;
    size_t srclen = 0;
    int r = dc::decode_front(c, enc, len, n, false, sh, dec, &src, &srclen, err);
    if (w) *w = sh.w;
    if (h) *h = sh.h;
    if (r) return r;
    if (scale < 1 || scale > n || (scale & (scale - 1)))
        return (ie_set_error(c, "ieh_decode_image_scaled: the scale is not a power of two from 1 to the block size"), IE_EINVAL);
    const size_t ow = size_t(sh.w / scale), need = ow * size_t(sh.h / scale);
    if (need > cap) return IE_ECAP;
    if ((r = ie_decode_scaled(c, src, srclen, sh.payload_bit, sh.w, sh.h, 1, sh.rle, scale, out, ow, need, nullptr))) return r;
    return int64_t(need);
}

int64_t ieh_decode_images(ie_ctx* c, const uint8_t* enc, size_t enc_pitch, const uint64_t* len, int count, int n,
                          uint8_t* out, size_t cap, int* w, int* h) {
    if (!c) return IE_EINVAL;
    if (!enc || !len || !out || count < 1 || (n != 4 && n != 8))
        return (ie_set_error(c, "ieh_decode_images: null argument, count < 1 or a block size other than 4 or 8"), IE_EINVAL);
    return dc::decode_files(c, enc, enc_pitch, len, count, n, out, cap, w, h);
}

int64_t ieh_decode_video(ie_ctx* c, const uint8_t* enc, size_t len, int n, uint8_t* out, size_t cap, int* w, int* h,
                         int* frames) {
    if (!c || !enc || !out) return IE_EINVAL;
    dc::StreamHeader sh;
    std::vector<uint8_t> pix;
    std::string err;
    const int r = dc::decode_file(c, enc, len, n, true, sh, pix, err, cap);
    if (w) *w = sh.w;
    if (h) *h = sh.h;
    if (frames) *frames = sh.frames;
    if (r) return r;
    std::memcpy(out, pix.data(), pix.size());
    return int64_t(pix.size());
}

int ieh_vdec_open(ie_ctx* c, const uint8_t* enc, size_t len, int n, int motioncomp, int chunk_frames, int* w, int* h,
                  int* frames, int* gop, int* merange, ieh_vdec** out) {
    if (!c || !enc || !out) return IE_EINVAL;
    *out = nullptr;
    std::string err;
    ieh_vdec* d = nullptr;
    const int r = dc::vdec_open(c, enc, len, n, motioncomp != 0, chunk_frames, &d, err);
    if (r) return (ie_set_error(c, err.c_str()), r);
    if (w) *w = d->sh.w;
    if (h) *h = d->sh.h;
    if (frames) *frames = d->sh.frames;
    if (gop) *gop = d->sh.gop;
    if (merange) *merange = d->sh.merange;
    *out = d;
    return IE_OK;
}

int ieh_vdec_next(ieh_vdec* v, uint8_t* out, size_t cap, int* got) {
    if (!v || !got) return IE_EINVAL;
    *got = 0;
    if (!out) return (ie_set_error(v->c, "ieh_vdec_next: null out"), IE_EINVAL);
    std::string err;
    const int r = dc::vdec_next(v, out, cap, got, err);
    if (r) ie_set_error(v->c, err.c_str());
    return r;
}

int ieh_vdec_close(ieh_vdec* v) {
    dc::vdec_close(v);
    return IE_OK;
}

int64_t ieh_huffman_encode_device(ie_ctx* c, const uint8_t* din, size_t n, uint8_t* dout, size_t cap) {
    if (!c || (!din && n) || !dout) return IE_EINVAL;
    if ((n && !dc::is_device(c, din)) || !dc::is_device(c, dout)) return IE_EINVAL;
    dc::DeviceBuffer out(c, dout, cap);
    std::string err;
    return algo::huffman_device(c, din, n, out, err);
}

int ieh_huffman_encode_device_batch(ie_ctx* c, const uint8_t* din, size_t in_pitch, const uint64_t* n, int count,
                                    uint8_t* dout, size_t out_pitch, int64_t* bytes) {
    if (!c || !din || !n || count <= 0 || !dout || !bytes) return IE_EINVAL;
    if (!dc::is_device(c, din) || !dc::is_device(c, dout)) return IE_EINVAL;
    std::string err;
    return algo::huffman_device_batch(c, din, in_pitch, n, count, dout, out_pitch, bytes, err);
}

// The batched Huffman pass straight after ie_encode_images on the same context: the string
// lengths come from the encoder's end bits on the device (no size read-back in between).
int ieh_huffman_encode_after_encode(ie_ctx* c, const uint8_t* din, size_t in_pitch, int count, uint8_t* dout,
                                    size_t out_pitch, int64_t* bytes) {
    if (!c || !din || count <= 0 || !dout || !bytes) return IE_EINVAL;
    if (!dc::is_device(c, din) || !dc::is_device(c, dout)) return IE_EINVAL;
    std::string err;
    return algo::huffman_device_batch(c, din, in_pitch, nullptr, count, dout, out_pitch, bytes, err,
                                      ie_last_end_bits(c));
}

// Pipelined form: _begin launches the histogram of the images the last ie_encode_images call
// wrote (read back into slot 0 or 1) and returns at once; _finish (same din / pitch / count / slot)
// builds the trees and launches the pack.  Issue batch i+1's encode and _begin before batch i's
// _finish and the host's tree builds overlap the device's encode.
int ieh_huffman_begin_after_encode(ie_ctx* c, const uint8_t* din, size_t in_pitch, int count, int slot) {
    if (!c || !din || count <= 0 || !dc::is_device(c, din)) return IE_EINVAL;
    return ie_huffman_hist_batch_ends_async(c, din, in_pitch, ie_last_end_bits(c), count, slot);
}

int ieh_huffman_finish_after_encode(ie_ctx* c, const uint8_t* din, size_t in_pitch, int count, int slot, uint8_t* dout,
                                    size_t out_pitch, int64_t* bytes) {
    if (!c || !din || count <= 0 || !dout || !bytes) return IE_EINVAL;
    if (!dc::is_device(c, din) || !dc::is_device(c, dout)) return IE_EINVAL;
    std::string err;
    return algo::huffman_device_batch_finish(c, din, in_pitch, count, slot, dout, out_pitch, bytes, err);
}

void ieh_release(ie_ctx* c) {
    std::lock_guard<std::mutex> lk(dc::g_mu);
    dc::g_scratch.erase(c);
}

// The Huffman decode alone (Huffman.cpp:354-402): returns the decoded byte count, or 0 with
// *passthrough = 1 for a stream without a dictionary; IE_ECAP if cap is too small.
// The dictionary of a Huffman-coded stream as the device decode's prefix table (32768 entries) and
// the code stream's first bit; returns 1 when the stream carries no dictionary (passthrough).
int ieh_huffman_table(const uint8_t* in, size_t n, uint16_t* lut, uint64_t* start_bit) {
    if ((!in && n) || !lut || !start_bit) return IE_EINVAL;
    bool pass = false;
    size_t from = 0;
    const int r = algo::Huffman::decode_table(in, n, lut, pass, from);
    if (r) return r;
    *start_bit = from;
    return pass ? 1 : 0;
}

int64_t ieh_huffman_decode(ie_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap, int* passthrough) {
    if (!c || (!in && n) || !out) return IE_EINVAL;
    std::vector<uint8_t> v;
    bool pass = false;
    size_t start = 0;
    const int r = algo::Huffman::decode(c, in, n, v, pass, start);
    if (r) return r;
    if (passthrough) *passthrough = pass ? 1 : 0;
    if (v.size() > cap) return IE_ECAP;
    if (!v.empty()) std::memcpy(out, v.data(), v.size());
    return int64_t(v.size());
}

int64_t ieh_huffman_encode(ie_ctx* c, const uint8_t* in, size_t n, uint8_t* out, size_t cap) {
    if (!c || (!in && n) || !out) return IE_EINVAL;
    std::vector<uint8_t> v;
    const int r = algo::Huffman::encode(c, in, n, v);
    if (r) return r;
    if (v.size() > cap) return IE_ECAP;
    std::memcpy(out, v.data(), v.size());
    return int64_t(v.size());
}

}  // extern "C"
