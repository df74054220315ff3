/* include/ie_hip.h -- the drop-in boundary: a C-ABI over the MI355X (gfx950) block codec.
 *
 * libie_hip.so replaces the LOOP BODY of the reference's frame encoders, i.e. everything between
 * "blocks exist" and "payload bits are in the writer":
 *
 *   dc::ImageEncoder::process      ImageEncoder.cpp:96-147  (DCT+quant, RLE build, serial emission)
 *   dc::Frame::process (I-frame)   Frame.cpp:129-159 + Frame::streamEncoded Frame.cpp:31-45
 *   algo::Huffman<>::encode        Huffman.cpp:233-344      (histogram + re-encode; the tree build
 *                                                            stays on the host, see ie_huffman_*)
 *   dc::ImageDecoder::process      ImageDecoder.cpp:55-122  (parse + IDCT + clamp; ie_decode_*)
 *
 * A per-block C call would cross the host/device boundary 518 400 times per 4K frame, so the
 * boundary is frame-batch level.  dc::Block<> has no counterpart here or in the host library
 * (include/ie_host.hpp, which mirrors ImageProcessor / MatrixReader / the encoders and decoders):
 * only the reference's own Block.o, linked into the drop-in builds of integration/, keeps that API
 * ("Why there is no dc::Block<N>").
 *
 * Conventions
 *   - Every function returns IE_OK (0) or a negative IE_E* code; ie_last_error() describes it.
 *     No C++ exception crosses this boundary.
 *   - Pixel and stream pointers may be host or device (hipMalloc) memory; the library detects
 *     which (hipPointerGetAttributes).  With device pointers and NULL result pointers every call is
 *     asynchronous on the context's stream.
 *   - Streams are MSB-first (bit k = bit 7-k%8 of byte k/8, BitStream.cpp:61-77).  The library
 *     only ORs bits in from `start_bit` on and never changes earlier bits, so a caller can write
 *     the settings header with its own BitStreamWriter and hand over start_bit = header length.
 *     Bits from start_bit on must be zero (the reference's writer buffer is zero-initialised,
 *     utils.hpp:443-446).  Device output buffers are written in whole 32-bit words: size them
 *     with ie_stream_bound().
 *   - One context per device, not internally locked; one stream per context.
 */
#ifndef IE_HIP_H
#define IE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ie_ctx ie_ctx;

enum {
    IE_OK = 0,
    IE_EINVAL = -1,    /* bad argument: N not 4|8, W%N or H%N != 0, W/H > 32767 (15-bit DIM_BITS) */
    IE_ECAP = -2,      /* output capacity too small */
    IE_EHIP = -3,      /* HIP runtime error */
    IE_ENOQUANT = -4,  /* ie_set_quant not called */
    IE_EFORMAT = -5,   /* malformed encoded stream */
    IE_EDEVICE = -6,   /* device-side protocol error (look-back timeout) */
};

enum {
    IE_MODE_FAST = 0,  /* separable FP32 DCT + exact FP64 re-evaluation of near-tie coefficients */
    IE_MODE_EXACT = 1, /* every coefficient in the reference's FP64 operation order */
};

/* Context lifetime.  device = HIP device ordinal. */
int ie_create(int device, ie_ctx** out);
int ie_destroy(ie_ctx* ctx);
const char* ie_last_error(const ie_ctx* ctx);
/* Record msg as the context's last error: for a layer above this ABI (libie_host.so) whose callers
 * read ie_last_error. */
int ie_set_error(ie_ctx* ctx, const char* msg);
/* Run on an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL restores
 * the context's own stream. */
int ie_set_stream(ie_ctx* ctx, void* hip_stream);
/* Wait for the context's stream, then check the device error counters: IE_EDEVICE if a tile
 * look-back timed out in any launch that returned without a read-back (asynchronous encodes,
 * packs, bit copies) since the last check -- that launch's output is invalid.  Later launches
 * then order their tiles by an atomic ticket.  Call it after a pipeline of asynchronous calls. */
int ie_sync(ie_ctx* ctx);

/* Quantisation matrix, n x n row-major uint16 (MatrixReader<N>::read, MatrixReader.cpp:65-134;
 * used as double[] via getData, :195-198).  n = 4 or 8 (the reference's compile-time
 * dc::BlockSize, Block.hpp:13, becomes a runtime parameter).  The host builds the DCT cos table
 * with std::cos in the reference's exact expression (algo.cpp:312,318-319).  q[k] must be > 0. */
int ie_set_quant(ie_ctx* ctx, const uint16_t* q, int n);

/* The cos table of the current quant matrix as the kernels use it, read back from the device:
 * out[u*n + i] = std::cos(((2.0*i + 1.0) * u) * (M_PI_2 / n)) evaluated by THIS host's libm when
 * ie_set_quant ran (algo.cpp:312,318-319), n*n doubles.  Lets a caller pin the machine's libm
 * against the reference's values (tests/golden/cos_table.json). */
int ie_cos_table(ie_ctx* ctx, double* out);

/* Upper bound in bytes of an output buffer for nframes frames of w x h encoded from start_bit
 * (4 + 17*16 bits per 4x4 block, 4 + 65*16 per 8x8 block, rounded up to whole 32-bit words). */
size_t ie_stream_bound(int w, int h, int n, int nframes, uint64_t start_bit);

/* Encode nframes frames as ONE bit-contiguous stream of block records (the gop=1 video payload
 * of Frame.cpp:31-45 / VideoEncoder.cpp:83-91; nframes = 1 is ImageEncoder's payload).
 *   y            frame f row r starts at y + f*frame_pitch + r*stride
 *   use_rle      Block::streamEncoded's use_rle (Block.cpp:372-413)
 *   mode         IE_MODE_FAST or IE_MODE_EXACT (identical output)
 *   out          stream buffer; records are appended from bit start_bit
 *   frame_bits   optional [nframes]: payload bits of each frame
 *   end_bit      optional: bit position after the last record
 * Replaces ImageEncoder.cpp:96-147 and the frame loop of VideoEncoder.cpp:83-91. */
int ie_encode_frames(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch,
                     int nframes, int use_rle, int mode, uint8_t* out, size_t out_cap,
                     uint64_t start_bit, uint64_t* frame_bits, uint64_t* end_bit);

/* Videos with P-frames (gop > 1; VideoEncoder.cpp:22-107, VideoBase.cpp:96-122, Frame.cpp:129-247):
 * frame f is an I-frame when f % gop == 0 (its payload = ie_encode_frames'), every other frame a
 * P-frame against the previous frame as the reference leaves it: per 16x16 macroblock a SAD pattern
 * search within merange (Block.cpp:267-339, algo.cpp:90-139), its motion vector (bits_needed(merange)
 * bits per component, Block.cpp:415-423), then the records of the 4x4 microblocks' coded prediction
 * error (ImageBase.cpp:266-306) -- 8x8 blocks carry the vectors only (the reference's
 * micro_per_macro_row is 0 there, ImageBase.cpp:271).  Replaces the frame loop of
 * VideoEncoder.cpp:83-91 for any gop; gop = 1 equals ie_encode_frames.  Arguments as
 * ie_encode_frames; out holds ie_gop_stream_bound() bytes.  IE_EINVAL for P-frames with W % 16 != 0
 * and H >= 32 (the reference reads misplaced, overlapping macroblocks there, ImageBase.cpp:223-227). */
size_t ie_gop_stream_bound(int w, int h, int n, int nframes, int merange, uint64_t start_bit);
int ie_encode_gop(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                  int gop, int merange, int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit,
                  uint64_t* frame_bits, uint64_t* end_bit);

/* ie_encode_gop with the video's groups of pictures encoded side by side: the same arguments, the
 * same ie_gop_stream_bound() capacity, host or device y and out, the same checks in the same order
 * with the same codes, and the same out bytes, frame_bits[] and *end_bit, bit for bit.  An I-frame
 * resets the prediction, so group g (frames g*gop .. g*gop + gop - 1) takes nothing from the groups
 * before it but the bit its payload starts at.  With G = ceil(nframes / gop) groups:
 *  - step 0 encodes the G I-frames as one batch of independent images (the launch of
 *    ie_encode_images), step j = 1 .. gop - 1 the j-th frame of every group that has one (one set
 *    of P-frame launches whose second grid dimension is the group); every group writes a private,
 *    zeroed slot of ie_gop_stream_bound(w, h, n, gop, merange, 0) bytes from bit 0;
 *  - a splice moves group g's bits to out at start_bit + the lengths of the groups before it
 *    (interior words stored, a group's first and last word ORed: out must be zero from start_bit
 *    on, the rule above) and fills the frames' position table.
 * The launch sequence is as deep as gop, not nframes.  One host synchronisation per call: the read
 * of the position table and the error counters.  A look-back timeout in an I-frame batch is
 * handled as in ie_encode_gop (a device out cleared from start_bit on, the video redone in ticket
 * mode).  Scratch per group: the slot, two reconstructed frames (2*w*h bytes), 32 bytes of
 * coefficients and 4 bytes of record length per 4x4 block, the record tiles' sums.  A video whose
 * scratch would exceed 1 GiB (or with more than 65535 groups) runs as waves of groups, one after
 * another on the stream, each wave's splice starting at the previous wave's end bit read on the
 * device -- still one synchronisation at the end; the environment variable IE_GOP_BATCH_MAX (read
 * on every call) lowers the wave size in groups further.  With gop <= 1 or fewer than two groups
 * the call is ie_encode_gop. */
int ie_encode_gop_groups(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                         int gop, int merange, int use_rle, int mode, uint8_t* out, size_t out_cap, uint64_t start_bit,
                         uint64_t* frame_bits, uint64_t* end_bit);

/* Encode nframes INDEPENDENT images in one launch (an image-server batch): image f's records
 * go to out + f*out_pitch from bit start_bit (each image carries its own header region).
 * end_bits optional [nframes].  out_pitch must be a multiple of 4 bytes. */
int ie_encode_images(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch,
                     int nframes, int use_rle, int mode, uint8_t* out, size_t out_pitch,
                     uint64_t start_bit, uint64_t* end_bits);

/* ie_encode_images (device output) that also counts the bytes of every image's stream -- the
 * caller's header words included, bytes [0, ceil(end_bit / 8)) -- while storing them: the counts
 * stay on the device for the next ie_huffman_hist_batch_ends_async over the same batch, which
 * then skips its own histogram pass (Huffman.cpp:237-243 without re-reading the stream).  MODE_EXACT,
 * 8x8 blocks or host output: a plain ie_encode_images (the histogram pass counts later).  No end bits are
 * returned (ie_last_end_bits holds them on the device). */
int ie_encode_images_counted(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch,
                             int nframes, int use_rle, int mode, uint8_t* out, size_t out_pitch, uint64_t start_bit);

/* Quantised DCT coefficients only (Block::processDCTDivQ, Block.cpp:139-153): coef receives
 * nframes * (w/n) * (h/n) blocks of n*n int16 in natural (row-major) order, block raster order.
 * coef may be host or device memory.  Diagnostic / analysis entry point. */
int ie_quantize_frames(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch,
                       int nframes, int mode, int16_t* coef);

/* Fallback statistics of the last FAST-mode encode launch: FP64 re-evaluation requests (one per
 * structural coefficient at a tie, one per block with another coefficient near a tie). */
int ie_last_fallbacks(ie_ctx* ctx, uint64_t* count);

/* "How big will this be?" -- the payload bits of every frame under nq candidate quantisation
 * matrices, from ONE pass over the pixels and without writing a stream (rate control: the matrix
 * travels in every file's header, so a file written with any matrix is a valid file).
 *   y, w, h, stride, frame_pitch, nframes   as ie_encode_frames (y host or device memory); the same
 *                checks with the same codes, IE_ENOQUANT before any ie_set_quant (the block size n
 *                and the transform tables come from it)
 *   q            host array of nq matrices, n*n uint16 each, row-major, n = the block size of the
 *                last ie_set_quant
 *   bits         nq * nframes entries, host or device (8-byte aligned) memory
 * bits[m*nframes + f] equals the frame_bits[f] that ie_encode_frames returns for these frames after
 * ie_set_quant(ctx, q + m*n*n, n), in either mode and for either use_rle: the unquantised
 * coefficient is formed once in the reference's FP64 order (algo.cpp:314-325), every candidate
 * divides (IEEE), rounds half away from zero and sizes the record by Block.cpp:186-232, :383-397.
 *  - IE_EINVAL: nq < 1, nq > IE_PROBE_MAX, or a matrix entry equal to 0 (ie_last_error names the
 *    matrix index).
 *  - The context's own matrix, tables and ie_last_end_bits are left exactly as they were: an encode
 *    after a probe equals the encode before it.
 *  - With a device `bits` the call is asynchronous on the context's stream (bits is zeroed there,
 *    the candidates go through pinned memory, then the launch).  With a host `bits` it
 *    synchronises once and reads the sums back in one copy.  Host frames are staged through the
 *    context's input buffer. */
enum { IE_PROBE_MAX = 64 };
int ie_probe_sizes(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch,
                   int nframes, int use_rle, const uint16_t* q, int nq, uint64_t* bits);

/* ---- Distortion probe: ie_probe_sizes' pass, and with it the squared error of the decoded pixels
 * of every frame under every candidate ("how good will it look?"), without writing or parsing a bit.
 *   y .. nq      as ie_probe_sizes: the same arguments, checks, error codes and their order
 *   sse          required: nq * nframes entries, host or device (8-byte aligned) memory
 *   bits         optional (NULL: not wanted): the same shape and memory rules; receives exactly what
 *                ie_probe_sizes writes.  bits and sse are both host or both device memory: a mix is
 *                IE_EINVAL.
 * sse[m*nframes + f] = the sum over the pixels of frame f of (d - y)^2, d the pixel that
 * ie_decode_frames writes for the stream that ie_encode_frames writes after ie_set_quant(ctx,
 * q + m*n*n, n), with the same use_rle, in either mode.  It is an integer and exact: per block the
 * kernel restates the quantised values (as the sizes probe), the one lossy rule of the stream (with
 * use_rle a record of length N*N whose zig-zag value N*N-2 is zero loses its last value,
 * Block.cpp:388-390), Y = double(v) * q, temp[ij] = temp[ij] + R[uv][ij] * Y[uv] over uv ascending
 * (algo.cpp:348-358, un-contracted), and x = temp + 128.0 clamped to [0, 255] and truncated
 * (Block.cpp:100-107).
 *  - The context's matrix, tables, chain state and ie_last_end_bits are left as they were.
 *  - With device results the call is asynchronous on the context's stream (the results are zeroed
 *    there).  With host results it synchronises once and reads both arrays back in one copy. */
int ie_probe_rd(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch,
                int nframes, int use_rle, const uint16_t* q, int nq, uint64_t* bits, uint64_t* sse);

/* ---- Size probe for videos with P-frames: ie_probe_sizes' question for ie_encode_gop.
 *   y .. nframes, gop, merange, use_rle   as ie_encode_gop (y host or device memory) and its checks
 *                with its codes, the output capacity apart: dimensions, merange in [0, 32767],
 *                frames, P-frames with W % 16 != 0 and H >= 32; then ie_probe_sizes' checks of nq
 *                and of zero matrix entries
 *   q, nq, bits  as ie_probe_sizes
 * bits[m*nframes + f] equals the frame_bits[f] that ie_encode_gop (and ie_encode_gop_groups) returns
 * for these frames after ie_set_quant(ctx, q + m*n*n, n), in either mode.  gop <= 1 or nframes == 1
 * is ie_probe_sizes.  I-frames (f % gop == 0) are sized by ie_probe_sizes' kernel.  P-frames with 4x4
 * blocks run the encoder's macroblock steps per candidate -- search, FP64 transform of the
 * prediction error, round((acc * S) / q), record sizes, inverse, reconstruction -- and emit nothing;
 * the first P-frame of a group predicts from the I-frame's source pixels, which all candidates
 * share, so its search and unquantised coefficients are formed once.  The launches are as deep as
 * gop, not nframes.  P-frames with 8x8 blocks carry vectors only: (w/16)*(h/16)*2*bits(merange).
 *  - Scratch: two reconstructed frames per (group, candidate) pair, owned by the context.  A call
 *    that would need more than 1 GiB runs as waves on the stream: whole groups with all candidates
 *    while they fit, else one group at a time with chunks of candidates.  IE_PROBE_GOP_MAX (read on
 *    every call) lowers the pairs per wave; it never changes the result.
 *  - Device `bits`: asynchronous on the context's stream (bits is zeroed there).  Host `bits`: one
 *    synchronisation and one read-back, however many waves run.
 *  - The context's matrix, tables, chain state, ie_last_end_bits and the encoders' gop scratch are
 *    left as they were: an ie_encode_gop after a probe equals the one before it. */
int ie_probe_gop(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                 int gop, int merange, int use_rle, const uint16_t* q, int nq, uint64_t* bits);

/* ---- Distortion probe for videos with P-frames: ie_probe_rd's question for ie_encode_gop +
 * ie_decode_gop.
 *   y .. use_rle, q, nq   as ie_probe_gop: the same checks, order and codes.  Then: a call with
 *                P-frames (gop > 1 and nframes > 1) needs W % 16 == 0 and H % 16 == 0 (ie_decode_gop's
 *                rule: what it refuses has no decoded pixels), and 4x4 blocks -- an 8x8 P-frame
 *                stream does not decode (ie_encode_gop writes no microblock records there,
 *                ie_decode_gop reads one per microblock), so there is nothing to measure: IE_EINVAL.
 *   motioncomp   the decoder setting the result is judged for, as in ie_decode_gop
 *   sse          required: nq * nframes entries, host or device (8-byte aligned) memory
 *   bits         optional (NULL: not wanted): receives exactly what ie_probe_gop writes.  bits and
 *                sse are both host or both device memory: a mix is IE_EINVAL.
 * sse[m*nframes + f] = the sum over frame f's w*h pixels of (d - y)^2, d the pixel that
 * ie_decode_gop(.., gop, merange, use_rle, motioncomp, ..) writes for the stream that ie_encode_gop
 * writes after ie_set_quant(ctx, q + m*n*n, n), in either mode: an exact integer.  gop <= 1 or
 * nframes == 1 is ie_probe_rd.
 * The decoder's frames are not the encoder's reconstructions.  The encoder's first P-frame of a
 * group predicts from the I-frame's source, the decoder copies from the lossy decoded I-frame; the
 * encoder rebuilds a P-frame from the quantised values, the decoder from the record after the one
 * lossy rule of the stream (see ie_probe_rd); the decoder reads the vector in bits(merange) bits.
 * So the probe carries both chains per candidate: the I-frames go through ie_probe_rd's kernel,
 * which also stores every candidate's decoded pixels; the P-frames through ie_probe_gop's macroblock
 * pass, which also forms the decoder's pixel (motioncomp: copied + (sum + 128), clamped and
 * truncated; else the copied pixel) and adds its squared error.
 *  - Scratch: four frames per (group, candidate) pair -- two reconstructions, two decoded frames --
 *    in a buffer of its own.  The 1 GiB wave rule and IE_PROBE_GOP_MAX work as in ie_probe_gop and
 *    never change a result.  The launches are as deep as gop.
 *  - Device results: asynchronous on the context's stream.  Host results: one synchronisation and
 *    one read-back.
 *  - The context's matrix, tables, chain state, ie_last_end_bits, the encoders' gop scratch and
 *    ie_probe_gop's scratch are left as they were. */
int ie_probe_gop_rd(ie_ctx* ctx, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                    int gop, int merange, int use_rle, int motioncomp, const uint16_t* q, int nq,
                    uint64_t* bits, uint64_t* sse);

/* ---- Device memory on the context's stream (for hosts that keep streams device-resident
 * between stages, e.g. the host library's encode -> Huffman pipeline).  ie_memcpy infers the
 * direction of each pointer and is asynchronous only when both are device memory. */
int ie_malloc(ie_ctx* ctx, size_t bytes, void** out);
int ie_free(ie_ctx* ctx, void* p);
int ie_memcpy(ie_ctx* ctx, void* dst, const void* src, size_t bytes);
int ie_memset(ie_ctx* ctx, void* dst, int value, size_t bytes);
/* 1 if p is device (hipMalloc) memory, 0 otherwise. */
int ie_is_device_ptr(const void* p);

/* ---- Streamed host path (the reference reads / writes whole files: utils.hpp:352-402,
 * VideoBase.cpp:6-19) -------------------------------------------------------------------------
 * ie_encode_images / ie_encode_frames with host frames AND a host stream buffer and nframes > 1
 * stream the batch through the device in chunks of a few frames: the H2D of chunk k+1, the encode
 * of chunk k and the D2H of chunk k-1 run concurrently on three HIP streams (PCIe full duplex),
 * through two device and two pinned host slots per direction.  Pinned caller buffers are DMA'd
 * directly, pageable ones through the pinned slots.  Page-locked host memory for such buffers: */
int ie_host_alloc(ie_ctx* ctx, size_t bytes, void** out);
int ie_host_free(ie_ctx* ctx, void* p);

/* Streamed video payload, gop=1 (Frame.cpp:31-45 / VideoEncoder.cpp:83-91 for frames that arrive
 * over time, e.g. read from a .raw/YUV420 file chunk by chunk): ONE bit-contiguous stream grown on
 * the device.  open: `head` holds the caller's bytes [0, ceil(start_bit/8)) (the settings header;
 * bits from start_bit on are ignored), max_frames bounds the device stream.  push: host frames
 * (frame f row r at frames + f*frame_pitch + r*stride), copied and encoded asynchronously, each
 * chunk continuing the chain from the previous chunk's end ON THE DEVICE (no host round trip);
 * pageable frames may be reused when push returns, pinned ones are DMA'd asynchronously and may
 * be reused once the NEXT push (or finish) returns (double-buffered readers alternate two).
 * pull: the whole bytes finished so far that were not pulled yet (from byte 0, the head included)
 * into dst (*nbytes of them), while later chunks still encode.  finish: waits, checks the device
 * error counters, copies the remaining bytes (last byte zero-padded) to dst when dst != NULL, and
 * returns the end bit and optionally each frame's payload bits.  ie_vstream_device: the device
 * stream (valid until close; complete after finish), e.g. for the device Huffman pass.  One open
 * stream per context at a time; other calls on the context between pushes are allowed.
 *
 * ie_vstream_open_gop: the same stream for a video with P-frames (gop > 1; with gop <= 1 the call
 * is ie_vstream_open).  push, pull, finish, device and close serve both kinds with the contract
 * above.  For ANY partition of the video's frames into pushes, the bytes (all pulls, then finish's
 * copy; also the device stream after finish), *end_bit and frame_bits[] equal ie_encode_gop's on
 * the whole video with the same start_bit and the same bits before it.  Checks: ie_vstream_open's,
 * then ie_encode_gop's with the same codes (merange in [0, 32767]; IE_EINVAL for P-frames with
 * W % 16 != 0 and H >= 32).  The device stream holds ie_gop_stream_bound(w, h, n, max_frames,
 * merange, start_bit) bytes, zeroed from the head on at open.  A chunk is Gc whole groups of
 * pictures (Gc * gop frames): frames gather across pushes in one of two device input slots (pushes
 * need not align with groups), a full slot is encoded as one wave of ie_encode_gop_groups whose
 * splice starts at the previous chunk's end bit read on the device, and finish encodes what is
 * left (its last group may be short).  Gc: IE_CHUNK_MB's pixel target (default 8 MiB), at most a
 * wave of ie_encode_gop_groups (1 GiB of scratch, 65535 groups, IE_GOP_BATCH_MAX), at least 1; all
 * read at open, none changes the output.  pull hands out the whole bytes up to the end of the
 * last finished chunk; a later chunk only adds bits to a byte that is not whole yet.  A look-back
 * timeout makes finish return IE_EDEVICE: earlier chunks' frames are gone, nothing is redone.  The
 * stream keeps its own table of frame positions, so an ie_encode_gop between pushes is harmless. */
typedef struct ie_vstream ie_vstream;
int ie_vstream_open(ie_ctx* ctx, int w, int h, size_t stride, size_t frame_pitch, int use_rle, int mode,
                    const uint8_t* head, uint64_t start_bit, int max_frames, ie_vstream** out);
int ie_vstream_open_gop(ie_ctx* ctx, int w, int h, size_t stride, size_t frame_pitch, int gop, int merange,
                        int use_rle, int mode, const uint8_t* head, uint64_t start_bit, int max_frames,
                        ie_vstream** out);
int ie_vstream_push(ie_vstream* v, const uint8_t* frames, int nframes);
int ie_vstream_pull(ie_vstream* v, uint8_t* dst, size_t cap, size_t* nbytes);
int ie_vstream_finish(ie_vstream* v, uint8_t* dst, size_t cap, size_t* nbytes, uint64_t* end_bit,
                      uint64_t* frame_bits);
const uint8_t* ie_vstream_device(const ie_vstream* v);
int ie_vstream_close(ie_vstream* v);

/* ---- Huffman post-pass (config 5; Huffman.cpp:233-344) ----------------------------------
 * hist[b] = occurrences of byte value b; first_pos[b] = index of its first occurrence
 * (UINT64_MAX if absent).  The first-occurrence order is the insertion order of the reference's
 * std::unordered_map (Huffman.cpp:237-243), which the host needs to replay the tree build. */
int ie_huffman_hist(ie_ctx* ctx, const uint8_t* bytes, size_t n, uint32_t* hist, uint64_t* first_pos);

/* Re-encode n bytes with a code table (code[b] right-aligned in len[b] bits, len <= 32),
 * appending from start_bit of out (Huffman.cpp:314-319).  end_bit optional. */
int ie_huffman_pack(ie_ctx* ctx, const uint8_t* bytes, size_t n, const uint32_t* code, const uint8_t* len,
                    uint8_t* out, size_t out_cap, uint64_t start_bit, uint64_t* end_bit);

/* Batched Huffman post-pass over `count` device-resident byte strings (one encoded image each):
 * string k is n[k] bytes at in + k*in_pitch (n: host array).  Replaces the per-image
 * Huffman.cpp:237-243 histogram loop; hist/first_pos hold count*256 entries (string k at 256*k),
 * host or device memory.  One launch for the whole batch. */
int ie_huffman_hist_batch(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* n, int count,
                          uint32_t* hist, uint64_t* first_pos);

/* The device array of per-image end bits of the last ie_encode_images launch (valid until the
 * next encode or Huffman call on the context; stream-ordered). */
const uint64_t* ie_last_end_bits(ie_ctx* ctx);

/* ie_huffman_hist_batch with the string lengths taken on the device from stream end bits
 * (n[k] = ceil(end_bits[k] / 8), e.g. ie_last_end_bits): the encoder -> Huffman pipeline needs no
 * host round trip for the sizes.  The host can recover n[k] as the sum of string k's histogram. */
int ie_huffman_hist_batch_ends(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* end_bits,
                               int count, uint32_t* hist, uint64_t* first_pos);

/* The same, split for pipelining batches: _async launches the histogram and its read-back into
 * pinned slot `slot` (0 or 1) and returns at once; _wait blocks until that slot's read-back is
 * complete and copies out count*256 counts and first positions.  While the host builds the trees
 * of batch i (between _wait and ie_huffman_pack_batch), the device runs batch i+1's encode and
 * histogram.  Same reference interface as ie_huffman_hist_batch (Huffman.cpp:237-243). */
/* After ie_encode_images_counted over the same batch, _async is ONE launch that takes the
 * encoder's counts (and clears them for the next counted encode) and writes counts and first
 * positions straight into the pinned slot; a string with a value first seen past its first
 * 256 KiB is finished by _wait, so `in` must stay unchanged until _wait returns (the pack that
 * follows reads it anyway). */
int ie_huffman_hist_batch_ends_async(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* end_bits,
                                     int count, int slot);
int ie_huffman_hist_batch_wait(ie_ctx* ctx, int slot, uint32_t* hist, uint64_t* first_pos);

/* Batched re-encode (Huffman.cpp:314-319 for every string of the batch in one launch): string k
 * with the code table code/len[256*k ...] into out + k*out_pitch from bit start_bit[k].  The
 * bits before start_bit[k] (the dictionary, Huffman.cpp:283-311, or the '0' bit of the "no gain"
 * copy) come from prefix + k*prefix_pitch, so `out` needs no preparation; bits of the prefix
 * from start_bit[k] on are ignored.  in/out: device memory, out and out_pitch 4-byte aligned,
 * out_pitch >= (start_bit[k] + max_len_k * n[k] + 31) / 32 * 4.  Host arrays n, code, len,
 * prefix, start_bit are copied before the call returns.  end_bit (host, count entries) optional:
 * asking for it synchronises; without it the call is asynchronous on the context's stream. */
int ie_huffman_pack_batch(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* n, int count,
                          const uint32_t* code, const uint8_t* len, const uint8_t* prefix, size_t prefix_pitch,
                          uint8_t* out, size_t out_pitch, const uint64_t* start_bit, uint64_t* end_bit);

/* Device time of the last batched Huffman stage on the context's stream (HIP events around its
 * launches): stage 0 = the histogram / first-occurrence kernels of ie_huffman_hist_batch_ends_async,
 * stage 1 = the pack kernel of ie_huffman_pack_batch.  Only those two batched calls record the
 * events (two hipEventRecord each), and only while ie_set_stage_timing(ctx, 1) is in effect (off by
 * default: the timing events cost the pipelined C5 step about 15 us of device idle time); the
 * single-string ie_huffman_hist / ie_huffman_pack never do.  Waits for the stage to finish. */
int ie_last_stage_ms(ie_ctx* ctx, int stage, float* ms);
int ie_set_stage_timing(ie_ctx* ctx, int on);

/* Copy n bytes into out starting at bit start_bit, i.e. shifted by start_bit % 8 (the "no gain"
 * path of Huffman.cpp:329-341 writes '0' + the input: start_bit = 1).  Device input and output:
 * asynchronous on the context's stream, like an encode without sizes (checked at ie_sync). */
int ie_bitcopy(ie_ctx* ctx, const uint8_t* bytes, size_t n, uint8_t* out, size_t out_cap, uint64_t start_bit);

/* Huffman decode on the device (algo::Huffman<uint8_t>::decode, Huffman.cpp:354-402, replacing the
 * per-bit tree walk of Huffman.cpp:190-204): the symbols of the code stream `in` (len bytes, host or
 * device) from start_bit (just past the dictionary) to the END OF THE BUFFER -- the reference also
 * decodes the padding bits of the last byte, a code running past the end reads zero bits.  lut
 * (host or device): 32768 uint16 entries, lut[p] = sym | len << 8 for the code that prefixes the
 * 15-bit string p (len 0: none; codes are <= 15 bits, Huffman.cpp:41-42), built by the caller from
 * the dictionary.  out (host or device, out_cap bytes) receives the symbols; *nout their count
 * (also when IE_ECAP is returned).  IE_EFORMAT: a bit string that no code prefixes.  A device
 * stream (4-byte aligned) and a device lut are read in place, not copied; with a device out the
 * symbols are written as they are decoded, never past out_cap (on IE_ECAP the first out_cap
 * symbols are there), and the call synchronises once. */
/* The dictionary half of Huffman<uint8_t>::decode (buildTree, Huffman.cpp:120-173): parse the
 * dictionary of a Huffman-coded stream from bit start_bit of `in` (host memory, len bytes) into
 * ie_huffman_decode's prefix table lut (32768 entries); *code_start = the bit after its stop bit.
 * Returns 0, 1 when the stream has no dictionary (the data follows uncompressed from *code_start,
 * Huffman.cpp:361-371), or IE_EFORMAT when the dictionary runs past the buffer. */
int ie_huffman_table(const uint8_t* in, size_t len, uint64_t start_bit, uint16_t* lut, uint64_t* code_start);

int ie_huffman_decode(ie_ctx* ctx, const uint8_t* in, size_t len, uint64_t start_bit, const uint16_t* lut,
                      uint8_t* out, size_t out_cap, size_t* nout);

/* Huffman-decode `count` INDEPENDENT code streams in one set of launches (the decode half of
 * ie_huffman_pack_batch; it replaces a loop of ie_huffman_decode calls, that is a loop over
 * Huffman.cpp:354-402). Stream k is len[k] bytes at in + k*in_pitch; its code stream starts at bit
 * start_bit[k] (just past its dictionary: the dictionaries differ in length) and is decoded to the
 * END OF ITS BUFFER, padding bits included, exactly as ie_huffman_decode does. lut: count * 32768
 * uint16 entries, image k's prefix table (ie_huffman_table) at 32768*k. Image k's symbols go to
 * out + k*out_pitch, never past out_pitch bytes; nout[k] = its true symbol count, also when that
 * exceeds out_pitch; the bytes of a slot past min(nout[k], out_pitch) are left untouched.
 * len, start_bit, nout: host arrays of `count` entries. in, lut, out: host or device.
 *  - IE_EINVAL: count < 1, len[k] > in_pitch, start_bit[k] > 8*len[k] (nothing is decoded).
 *    start_bit[k] == 8*len[k] is an empty code stream: nout[k] = 0, no error.
 *  - One synchronisation and one device-to-host read per call: every image's total and flag pair
 *    come back together.  With a device `out` the symbols are written as they are decoded, before
 *    the totals are known (bounded by out_pitch); a host `out` adds the copy of the symbols, never a
 *    second table pass.
 *  - An image holding a bit string no code prefixes makes the call return IE_EFORMAT, with
 *    nout[k] = UINT64_MAX; an image with nout[k] > out_pitch makes it return IE_ECAP (the first
 *    out_pitch symbols are there).  The call returns the code of the LOWEST failing k and
 *    ie_last_error names that k; every other image's symbols and count are delivered as by a
 *    successful call (the contract of ie_decode_images).
 *  - A device `in` that is 4-byte aligned with in_pitch a multiple of 4 is read in place, and so
 *    is a device lut; anything else is first copied into context scratch, from host memory only
 *    the len[k] bytes of every image.
 *  - One chunk plan serves the batch: the chunk count comes from the longest code stream, and a
 *    shorter stream's trailing chunks hold no code.  Scratch is per image (about 2 bytes per stream
 *    bit of the longest stream).  A batch whose scratch would exceed 1 GiB runs as sub-batches one
 *    after another, still with one synchronisation at the end; the environment variable
 *    IE_DEC_BATCH_MAX (read on every call) lowers the sub-batch size in images further. */
int ie_huffman_decode_batch(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* len, int count,
                            const uint64_t* start_bit, const uint16_t* lut,
                            uint8_t* out, size_t out_pitch, uint64_t* nout);
/* The same call, which also returns the first head_bytes (<= out_pitch) bytes of every output slot
 * in host memory, heads + k*head_bytes, within the same synchronisation (ieh_decode_images reads
 * the settings headers of the decoded streams this way; the bytes past nout[k] are whatever the
 * slot held). */
int ie_huffman_decode_batch_heads(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* len, int count,
                                  const uint64_t* start_bit, const uint16_t* lut,
                                  uint8_t* out, size_t out_pitch, uint64_t* nout, uint8_t* heads, size_t head_bytes);

/* ---- Inverse path (ImageDecoder.cpp:55-122, Block.cpp:100-107,163-177,442-472) ------------
 * Decode nframes frames of block records starting at bit start_bit of `in` (len bytes) into
 * pixels (frame f row r at out + f*frame_pitch + r*stride).  Uses the quant matrix of
 * ie_set_quant.  end_bit optional. */
int ie_decode_frames(ie_ctx* ctx, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h,
                     int nframes, int use_rle, uint8_t* out, size_t stride, size_t frame_pitch,
                     uint64_t* end_bit);

/* Decode `count` INDEPENDENT images of w x h in one set of launches (the inverse of
 * ie_encode_images). Image k's stream is the bits [0, nbits[k]) of in + k*in_pitch, its first
 * record at start_bit (the same for every image: the settings header is the same); bits of the
 * slot at or past nbits[k] are ignored, whatever they hold. Image k's pixels go to
 * out + k*frame_pitch, row r at + r*stride. nbits: host array. in/out: host or device.
 * end_bits (host, optional, [count]): the bit after image k's last record, UINT64_MAX for an
 * image whose stream ends before its last block.
 *  - IE_EINVAL: the checks of ie_decode_frames (dimensions, stride, frame_pitch when count > 1),
 *    count < 1, nbits[k] > 8*in_pitch, start_bit > nbits[k].
 *  - One synchronisation per call: every image's record total and end bit come back in one read.
 *  - A truncated image k (fewer records than blocks, or its last record past nbits[k]) makes the
 *    call return IE_EFORMAT, ie_last_error naming the lowest such k, with end_bits[k] =
 *    UINT64_MAX; every other image's pixels and end bit are delivered as by a successful call
 *    (host and device out alike; the truncated image's pixels are unspecified).
 *  - A device `in` that is 16-byte aligned with in_pitch a multiple of 16 is read in place;
 *    anything else (host memory, another pitch or base) is first copied into such slots on the
 *    device, from host memory only the ceil(nbits[k]/8) bytes of every image.
 *  - Always the exact parse: ie_set_exact_parse(ctx, 0) does not affect this call, and
 *    ie_last_decode_spec returns 0 after it.  ie_last_decode_info then reports the chunks PER IMAGE
 *    (one chunk plan serves the batch: chunk length from the longest stream) and the composition
 *    levels.
 *  - Scratch is per image (about 23 MB for a 3840x2160 4x4 image).  A batch whose scratch would
 *    exceed 1 GiB runs as sub-batches one after another, still with one synchronisation at the
 *    end; the environment variable IE_DEC_BATCH_MAX (read on every call) lowers the sub-batch
 *    size in images further. */
int ie_decode_images(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                     uint64_t start_bit, int w, int h, int use_rle,
                     uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bits);

/* Region decode: only the pixels of the rectangle (x0, y0, rw, rh) -- columns x0 .. x0+rw-1, rows
 * y0 .. y0+rh-1 -- of every frame (ie_decode_region, the arguments of ie_decode_frames) or of every
 * image (ie_decode_images_region, the arguments of ie_decode_images; one rectangle for the batch).
 * `out` receives rw x rh pixels per frame or image: row r of frame f at out + f*frame_pitch +
 * r*stride, only the rw bytes of a row written, every other byte of `out` left untouched.  These
 * pixels equal, byte for byte, the same rows and columns of what ie_decode_frames (ie_decode_images)
 * writes for the same stream and arguments.  in/out: host or device.
 *  - The whole stream is parsed -- the records are a serial chain -- so *end_bit / end_bits[] are the
 *    full decode's, and a stream that ends before its last block is IE_EFORMAT with the full decode's
 *    message (ie_decode_images_region: the lowest such k named, end_bits[k] = UINT64_MAX, every other
 *    image's region and end bit delivered), also when the missing records lie outside the rectangle.
 *    What the rectangle saves is the inverse transform of the blocks outside it, the pixel stores
 *    and, for a host `out`, the copy: rows of rw bytes cross, nothing else.
 *  - Always the exact parse: ie_set_exact_parse(ctx, 0) does not affect these calls, and
 *    ie_last_decode_spec returns 0 after them.  ie_last_decode_info reports as for the full call.
 *  - Checks, in this order: NULL pointers (IE_EINVAL); IE_ENOQUANT and the dimension checks of
 *    ie_decode_frames on (w, h, nframes or count); the rectangle -- x0 >= 0, y0 >= 0, rw >= 1,
 *    rh >= 1, x0 + rw <= w, y0 + rh <= h, else IE_EINVAL with a message naming it; stride >= rw, and
 *    frame_pitch >= (rh-1)*stride + rw when there is more than one frame or image; then the
 *    start_bit (and nbits) checks of the full call.  Nothing is written after a failed check.
 *  - A rectangle equal to the whole frame is legal and equals the full decode.
 *  - One synchronisation per call.  The stream is staged as by the full call (an aligned device
 *    stream or batch of slots is read in place).  A host `out` is decoded into a packed buffer of
 *    the context, rw*rh bytes per frame; a device `out` is written in place.
 *    ie_decode_images_region keeps the 1 GiB sub-batch rule and IE_DEC_BATCH_MAX.
 *  - I-frames only.  A P-frame's motion vectors reach outside any rectangle, so a region of a gop > 1
 *    video needs the whole previous frame: decode it with ie_decode_gop / ie_vdec and crop. */
int ie_decode_region(ie_ctx* ctx, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h,
                     int nframes, int use_rle, int x0, int y0, int rw, int rh,
                     uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit);
int ie_decode_images_region(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                            uint64_t start_bit, int w, int h, int use_rle, int x0, int y0, int rw, int rh,
                            uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bits);

/* Scaled decode: every frame (ie_decode_scaled, the arguments of ie_decode_frames) or image
 * (ie_decode_images_scaled, the arguments of ie_decode_images) at 1/scale of its width and height:
 * the thumbnail out of the decode pass.  scale = s must be a power of two with 1 <= s <= N, N the
 * context's block size: 1, 2, 4 for 4x4 blocks and 1, 2, 4, 8 for 8x8.  `out` receives ow x oh
 * pixels per frame or image, ow = w/s, oh = h/s (exact: w and h are multiples of N): row r of frame
 * f at out + f*frame_pitch + r*stride, only the ow bytes of a row written, every other byte of `out`
 * left untouched.  in/out: host or device.
 *  - The pixel, exactly.  With `full` what ie_decode_frames (ie_decode_images) writes for the same
 *    stream and arguments,
 *      out[f][Y][X] = (sum over dy < s, dx < s of full[f][Y*s+dy][X*s+dx] + s*s/2) >> (2*log2 s):
 *    the box mean of the decoded integer pixels -- after +128, clamp and truncation -- rounded half
 *    up.  Nothing about the transform is approximated; the mean is not formed from the DC value or
 *    from the unclamped doubles.  scale = 1 equals the full decode byte for byte.
 *  - The whole stream is parsed, so *end_bit / end_bits[] are the full decode's, and a stream that
 *    ends before its last block is IE_EFORMAT with the full decode's message (ie_decode_images_scaled:
 *    the lowest such k named, end_bits[k] = UINT64_MAX, every other image delivered).  A host `out`
 *    receives nothing from an ie_decode_scaled call that returns IE_EFORMAT.  Every block is
 *    transformed; what a scale saves is stores and, for a host `out`, the copy: 1/s^2 of the bytes.
 *  - Always the exact parse: ie_set_exact_parse(ctx, 0) does not affect these calls, and
 *    ie_last_decode_spec returns 0 after them.  ie_last_decode_info reports as for the full call.
 *  - Checks, in this order: NULL pointers (IE_EINVAL); IE_ENOQUANT and the dimension checks of
 *    ie_decode_frames on (w, h, nframes or count); the scale, else IE_EINVAL with a message naming
 *    the scale; stride >= ow, and frame_pitch >= (oh-1)*stride + ow when there is more than one
 *    frame or image; then the start_bit (and nbits) checks of the full call.  Nothing is written
 *    after a failed check.
 *  - One synchronisation per call.  The stream is staged as by the full call (an aligned device
 *    stream or batch of slots is read in place).  A host `out` is decoded into a packed buffer of
 *    the context, ow*oh bytes per frame, and copied as rows of ow bytes; a device `out` is written
 *    in place.  ie_decode_images_scaled keeps the 1 GiB sub-batch rule and IE_DEC_BATCH_MAX.
 *  - I-frames only, as the region calls: a P-frame needs the whole previous frame at full size. */
int ie_decode_scaled(ie_ctx* ctx, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h,
                     int nframes, int use_rle, int scale,
                     uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bit);
int ie_decode_images_scaled(ie_ctx* ctx, const uint8_t* in, size_t in_pitch, const uint64_t* nbits, int count,
                            uint64_t start_bit, int w, int h, int use_rle, int scale,
                            uint8_t* out, size_t stride, size_t frame_pitch, uint64_t* end_bits);

/* Video payload with P-frames (VideoDecoder.cpp:28-58, Frame.cpp:47-127, Block.cpp:441-496): frame f
 * an I-frame when f % gop == 0 (decoded as ie_decode_frames), otherwise a P-frame: its motion vectors
 * (bits_needed(merange) bits each), the previous decoded frame's blocks at the clamped vectors copied
 * into place, then a record for every microblock whose decoded error (IDCT + 128) is added to the
 * copied pixels (motioncomp != 0) or read and dropped (motioncomp == 0).  W and H multiples of 16
 * when P-frames exist (IE_EINVAL otherwise).  end_bit optional. */
int ie_decode_gop(ie_ctx* ctx, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes,
                  int gop, int merange, int use_rle, int motioncomp, uint8_t* out, size_t stride,
                  size_t frame_pitch, uint64_t* end_bit);

/* Streamed video decode (the mirror of ie_vstream; VideoDecoder.cpp:28-58 for frames that leave as
 * they are decoded): ie_decode_gop's payload handed out in chunks of frames.  open: the stream `in`
 * (len bytes, host or device) with ie_decode_gop's arguments; gop <= 1 means every frame is an
 * I-frame.  chunk_frames: frames per chunk; 0 picks max(1, target / (w*h)) with IE_CHUNK_MB's pixel
 * target (default 8 MiB, read at open); the output does not depend on it.  next: the next frames,
 * at most max_frames of them (*got), frame i of the call at out + i*frame_pitch, its row r at
 * + r*stride, only the w bytes of a row written (out host or device; stride >= w, frame_pitch
 * covers a frame when max_frames > 1).  After the last frame next returns IE_OK with *got = 0.
 * info: the frames per chunk, the chunks enqueued and delivered so far (enqueued <= delivered + 2
 * at all times) and the end bit, UINT64_MAX until the last frame is out.  For ANY chunk_frames >= 1
 * and ANY partition of the video into next calls, the frames in order equal, byte for byte, what
 * ie_decode_gop writes for the whole stream with the same arguments, and the end bit equals its.
 *  - Checks at open: ie_decode_gop's in its order with its codes (IE_ENOQUANT, dimensions, merange
 *    in [0, 32767], P-frames only for W % 16 == 0 && H % 16 == 0, start_bit <= 8*len), then
 *    chunk_frames < 0 and a second open decoder on the context (one at a time): IE_EINVAL.
 *  - Pipeline: two device slots of chunk_frames frames.  open enqueues chunks 0 and 1; the next that
 *    hands out the last frame of chunk k enqueues chunk k+2 into the slot just freed (a host out:
 *    once chunk k's D2H is complete; a device out: behind the copy in stream order) before it waits
 *    for anything further, so chunk k+1 decodes while chunk k's frames cross.  A chunk starts at the
 *    end bit of the chunk before it, read on the device: one host synchronisation per chunk, the
 *    read of its positions and record totals.  With gop <= 1 a chunk is one exact parse of
 *    chunk_frames frames; with gop > 1 the per-frame launches of ie_decode_gop, a chunk's first
 *    P-frame reading its reference from the other slot.  A host out is written through a D2H stream
 *    of the decoder's own: directly when page-locked (ie_host_alloc), else through pinned staging.
 *  - Ownership: a host `in` (or an unaligned device one) is copied at open and may be freed when
 *    open returns; a 16-byte aligned device `in` is read in place and must stay valid until close.
 *    The decoder keeps its own copy of the quantisation tables and block size as they were at open,
 *    its positions and its slots: ie_set_quant with another matrix, or any other decode or encode
 *    on the context between two next calls, changes nothing.  Device memory: the two slots and the
 *    stream, whatever nframes is.  The context's stream must stay the same from open to close.
 *  - A stream that ends inside frame f (its vectors or its records): the next that reaches f hands
 *    out the frames before f (*got), returns IE_EFORMAT with ie_decode_gop's message, and every
 *    later next returns IE_EFORMAT with *got = 0.  (gop <= 1: the whole frames of a chunk are its
 *    record total / blocks per frame.)  max_frames < 1: IE_EINVAL.
 *  - close waits for the chunks still decoding; call it before ie_destroy. */
typedef struct ie_vdec ie_vdec;
int ie_vdec_open(ie_ctx* ctx, const uint8_t* in, size_t len, uint64_t start_bit, int w, int h, int nframes,
                 int gop, int merange, int use_rle, int motioncomp, int chunk_frames, ie_vdec** out);
int ie_vdec_next(ie_vdec* v, uint8_t* out, size_t stride, size_t frame_pitch, int max_frames, int* got);
int ie_vdec_info(const ie_vdec* v, int* chunk_frames, int* chunks_enqueued, int* chunks_delivered,
                 uint64_t* end_bit);
int ie_vdec_close(ie_vdec* v);

/* Chunks and composition levels of the last ie_decode_frames call's exact parse (after
 * ie_decode_images: the chunks per image) (diagnostics: the
 * stream is cut into chunks of about 32 (4x4) / 16 (8x8) records, each tabulated over every entry
 * offset; the tables are composed G at a time, level after level). */
int ie_last_decode_info(ie_ctx* ctx, int* chunks, int* levels);

/* Record-parse mode of ie_decode_frames / ie_decode_gop.  By default (exact != 0, any nonzero
 * value) the exact parse over composed transfer tables.  exact = 0: a call first parses
 * speculatively -- every chunk's entry is where a walk from its predecessor's first bit left it,
 * and the counting walks, each from its predecessor's speculative exit, verify every exit; on any
 * mismatch (periodic content, e.g. gradients) nothing is written and the exact parse runs.  Faster
 * only on flat content.
 * ie_set_spec_warm: the speculative parse's warm-up chunks (clamped to [0, 8], default 0) -- a
 * chunk's walk starts that many chunks earlier (the count pass's LDS bounds it further for long
 * chunks).  (Round 4 briefly encoded the warm-up as a negative `exact`; that meaning is gone: a
 * negative `exact` is nonzero, i.e. the exact parse, as before it.)
 * ie_last_decode_spec returns 1 when the last record decode was completed by the speculative
 * parse, 0 when by the exact one. */
int ie_set_exact_parse(ie_ctx* ctx, int exact);
int ie_set_spec_warm(ie_ctx* ctx, int warm);
int ie_last_decode_spec(ie_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
