// imageencoder_amd/csrc/ie_device.h -- structures shared by the host context (ie_capi.cpp) and
// the gfx950 kernels (ie_encode.hip, ie_encode4p.hip, ie_huffman.hip, ie_decode.hip,
// ie_decode_region.hip, ie_decode_scaled.hip, ie_huffman_decode.hip, ie_pframe.hip, ie_probe.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ie_dct.h"

namespace ie {

constexpr int kTPB = 256;  // threads per workgroup: 4 waves of 64

// Per-quant-matrix tables, built once on the host by ie_set_quant (ie_capi.cpp).
struct EncTables {
    // FP32 fast path (separable DCT, see encode_fast in ie_encode.hip)
    float cf[64];   // cf[u*N+i] = float(c[u][i])
    float g[64];    // float(S[uv] / q[uv])
    float thr[64];  // bound on |t32 - t_ref|; < 0: t32 exact (coefficient 0 only)
    float lim[64];  // 0.5 - thr: |t32 - rint(t32)| >= lim flags a possible rounding tie
    DctConsts dct;  // butterfly constants cos(k pi/16)
    Dct4Plan plan4; // 4x4 folded quotient transform (quot4)
    float lim_min;  // min of lim[k] over the non-structural coefficients: one compare per block
    int dc_exact;   // t[0] is exact in FP32 (q[0] a power of two): round it directly
    int rec_bits;   // largest record (bits) any block can produce with this matrix: sizes the tile image
    // 4x4 on the matrix pipe (encode4p_kernel, quot4j in ie_dct.h): the FP32 stage's constants, its
    // own tie limits (the tracked run of quot4j), and the i8 A fragment of every lane: lane l =
    // (r = l & 31, h = l >> 5) holds in byte 4i + j the weight of pixel (i, j) in J[rho], rho =
    // (r & 3) + 4 (r >> 3), when h == (r >> 2) & 1, else 0 -- so D register rho of a lane is J[rho]
    // of the lane's OWN block (C/D row = (reg & 3) + 8 (reg >> 2) + 4 h).
    Dct4JPlan plan4j;
    float lim4j[16];
    float lim_min4j;
    int dc_exact4j;
    // the same stage forming t + 1/2 (quot4j<true>): coefficient k is near a rounding tie when
    // fract(t + 1/2) <= dlo4h[k] or >= dhi4h[k] (2 x its tracked bound, rounded outward); the
    // non-structural coefficients share the loosest pair (dlo_max4h, dhi_min4h)
    float dlo4h[16], dhi4h[16];
    float dlo_max4h, dhi_min4h;
    int dc_exact4h;
    uint32_t mfma_w[64][4];
    // 4x4: P[16][16] then S, rq, qd of every coefficient, contiguous (the fix-up's LDS copy, staged
    // by DMA: 152 lanes x 16 bytes)
    double rows4[16 * 16 + 3 * 16];
    // the structural coefficients' rows P[k_s][*] (s = 0..2), then S, rq, qd of the three: the
    // fix-up's LDS copy, one contiguous block (3*NN + 9 doubles)
    double srow[3 * 64 + 9];
    // FP64 reference order (algo.cpp:309-331, Block.cpp:149-152)
    double S[64];   // C(u)*C(v)
    double qd[64];  // double(q[uv])
    double rq[64];  // 1/q when q is a power of two (exact), else 0 -> divide
    double c[64];   // c[u*N+i] (std::cos, algo.cpp:318-319)
    double P[64 * 64];  // P[uv*NN + ij] = c[u][i]*c[v][j]
    // inverse (algo.cpp:343-363): R[uv*NN + ij] = ((C(u)*C(v))*c[u][i])*c[v][j]
    double R[64 * 64];
};

// Division by a launch constant d (1 <= d < 2^31) for dividends n < 2^31, by a multiply-high:
// floor(n / d) = (mulhi(n, mul) + n) >> shr with shr = ceil(log2 d), mul = floor(2^32 (2^shr - d) / d) + 1
// (Granlund-Montgomery).  Built on the host (make_fastdiv), evaluated in scalar registers.
struct FastDiv {
    uint32_t d, mul, shr;
};
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f{d, 0u, 0u};
    while ((1ull << f.shr) < d) f.shr++;
    f.mul = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << f.shr) - d)) / d + 1);
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, uint32_t mul, uint32_t shr) {
    return (__umulhi(n, mul) + n) >> shr;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) { return fdiv(n, f.mul, f.shr); }

// One encode launch.  Tiles (workgroups) never straddle frames; a "chain" is the sequence of
// tiles whose bit offsets accumulate: the whole batch (concatenated stream) or one frame
// (independent images, segmented = 1).
struct EncArgs {
    const uint8_t* y;
    uint64_t stride, frame_pitch;
    int w, h, nframes;
    int bx, by;              // blocks per row / column
    int gpr;                 // thread groups per block row = ceil(bx / BPT)
    uint32_t gpr_magic;      // ceil(2^32 / gpr): exact floor(r / gpr) = mul_hi(r, magic) for r < gpr + 2^16
    int groups_per_frame;    // gpr * by
    int tiles_per_frame;     // ceil(groups_per_frame / encode_threads_per_tile())
    int ntiles;
    FastDiv div_frames, div_tpf, div_gpr;  // by nframes, tiles_per_frame, gpr
    int rle;
    int segmented;
    int vec_ok;              // kVecGroup | kVec16 (below); 0: rows are read byte by byte
    uint32_t* out;           // 4-byte aligned, word w = stream bytes [4w, 4w+4)
    uint64_t out_pitch_words;
    uint64_t start_bit;
    const uint64_t* start_dev;  // non-null: the chain starts at *start_dev (device; overrides start_bit)
    uint64_t* st;            // [3*ntiles] tile chain granules (ie_common.hpp)
    unsigned long long* ticket;  // nullptr: tiles in blockIdx order; else an atomic ticket
    unsigned long long ticket_base;
    uint32_t tag;            // epoch tag 1..255
    uint64_t* frame_start;   // [nframes] absolute start bit of each frame's payload
    uint64_t* chain_end;     // [nchains] absolute end bit
    unsigned* err;           // [0] look-back timeouts (atomic, only ever on a timeout)
    uint32_t* wave_fix;      // [ntiles * kTPB/64] FP64 fix-up requests per wave (plain stores, statistics)
    const EncTables* tab;
    int16_t* coef;           // optional: quantised coefficients, natural order, [nframes*bx*by][N*N]
    int ablate;              // profiling only (IE_ABLATE): 1 no FP64, 2 no emission, 4 no look-back, 8 no store, 16 no DCT, 128 no pixel loads
    uint64_t* stamps;        // profiling only (IE_STAMPS): [tile][kStamps] s_memtime per phase, thread 0
    int deep_lb;             // the launch does not fill the chip: look-back windows issued at once
    int rec_bits;            // = tab->rec_bits (host copy): launch_encode sizes the LDS tile image from it
    int tri;                 // 4x4: every bl <= 11 (from rec_bits): records emitted three coefficients per field
    int img_words;           // set by launch_encode
    // optional (segmented launches): per-frame byte histograms [nframes][256] of the stream bytes
    // [0, ceil(end/8)) -- header included -- ADDED to by the launch (the Huffman pass's counts)
    uint32_t* hist;
};

// EncArgs::vec_ok.  The frames' base, the row stride and (several frames) the frame pitch are all
// multiples of ...
constexpr int kVecGroup = 1;  // ... a group's row (4x4: 16 bytes, 8x8: 8): every group's row may be read with one load
constexpr int kVec16 = 2;     // ... 16 bytes: what a 16-byte LDS DMA requires of its source (implies kVecGroup)

constexpr int kStamps = 64;  // encode_kernel: [0, 16) by thread 0; encode4p_kernel: [4 waves][16] by each wave's lane 0
// chain-state words per tile (the host allocates; ie_common.hpp kGran must not exceed it)
constexpr int kStateWordsPerTile = 16;
// returns the FP64-statistics words per tile the launched kernel writes (EncArgs::wave_fix)
int launch_encode(const EncArgs& a, int n, bool exact, hipStream_t s);
// the wave-local 4x4 FAST encoder (ie_encode4p.hip); launch_encode checks its preconditions
int launch_encode4p(const EncArgs& a, hipStream_t s);
int encode_blocks_per_thread(int n);  // horizontally adjacent blocks per lane, Geo<N>::BPT (4x4: 4, 8x8: 1)
int encode_small_tiles();             // a launch of fewer tiles does not fill the chip (deep look-back)
void launch_word_scatter(const uint32_t* src, uint32_t* dst, uint64_t pitch_words, int n, hipStream_t s);
int encode_threads_per_tile();       // threads per encoder workgroup (= tile)

// ie_probe_sizes / ie_probe_rd (ie_probe.hip): the payload bits, and the squared error of the
// decoded pixels, of every frame under nq candidate matrices.
struct ProbeArgs {
    const uint8_t* y;
    uint64_t stride, frame_pitch;
    int bx, by, nframes;
    int rle;
    int vec_ok;              // rows may be read with 4-byte loads
    int nq;                  // 1 .. IE_PROBE_MAX
    const uint16_t* q;       // [nq][N*N] candidates in ZIG-ZAG order (device)
    const EncTables* tab;    // P, S and R of the block size (they do not depend on the matrix)
    unsigned long long* bits;  // [nq][nframes], zero before the launch: bits[m * nframes + f] is added to
    // launch_probe_rd_store alone (ie_probe_gop_rd's I-frames; the other launches never read these):
    // the sums of candidate m, frame f are added to bits / sse [m * out_m + f * out_f], and the
    // decoded pixels of the first dec_frames frames go to dec + f * f_dec + m * m_dec, [h][w] packed
    uint64_t out_m, out_f;
    uint8_t* dec;
    uint64_t f_dec, m_dec;
    int dec_frames;
};
void launch_probe_sizes(const ProbeArgs& a, int n, hipStream_t s);
// the distortion too: sse has the shape and rule of bits, which may then be nullptr
void launch_probe_rd(const ProbeArgs& a, unsigned long long* sse, int n, hipStream_t s);
int probe_rd_max_workgroups(int n);  // the grid of launch_probe_rd is min(tiles, this)
// launch_probe_rd for 4x4 blocks that also stores every candidate's decoded pixels (the fields
// above): four pixels to a store, so w % 4 == 0 and dec, f_dec, m_dec multiples of 4
void launch_probe_rd_store(const ProbeArgs& a, unsigned long long* sse, hipStream_t s);

struct PackArgs {            // Huffman re-encode / bit copy: one variable-length code per byte
    const uint8_t* in;
    uint64_t n;              // input bytes
    const uint32_t* code;    // [256]
    const uint8_t* len;      // [256]
    int ntiles;
    uint32_t* out;
    uint64_t start_bit;
    uint64_t* st;
    unsigned long long* ticket;
    unsigned long long ticket_base;
    uint32_t tag;
    uint64_t* chain_end;
    unsigned* err;
    // batch mode (count > 0): string k owns the tiles t with t % count == k (position t / count,
    // tiles[k] of them), one chain each; its bytes at in + k*in_pitch (n[k] of them), its code
    // table at code/len + 256*k, its output at out + k*out_pitch_words from bit start[k], the words
    // before that from prefix + k*prefix_pitch_words (e.g. the Huffman dictionary), its end bit in
    // chain_end[k].  ntiles = count * max_k tiles[k].
    int count;
    const uint64_t* tiles;       // [count]
    const uint64_t* bn;          // [count]
    const uint64_t* bstart;      // [count]
    uint64_t in_pitch, out_pitch_words, prefix_pitch_words;
    const uint32_t* prefix;
    int maxlen;                  // longest code in the table(s): picks the tile shape
};
// input bytes per pack tile for codes of at most maxlen bits (ie_huffman.hip)
int pack_tile_bytes(int maxlen);
void launch_pack(const PackArgs& a, hipStream_t s);
// ie_bitcopy: n bytes to stream bit start_bit of out (no scan, no look-back; ie_huffman.hip)
void launch_bitshift(const uint8_t* in, uint64_t n, uint32_t* out, uint64_t start_bit, hipStream_t s);
// hist / first (each optional, count*256): cleared to 0 / ~0 by the same launch
void launch_ends_to_bytes(const uint64_t* ends, uint64_t cap, int count, uint64_t* n, hipStream_t s,
                          uint32_t* hist = nullptr, unsigned long long* first = nullptr);
// unresolved: device scratch, one word per string
void launch_hist(const uint8_t* in, uint64_t n, uint32_t* hist, unsigned long long* first, unsigned* unresolved,
                 hipStream_t s);
// count strings at in + k*pitch, n[k] (device array) bytes each, maxn >= every n[k]:
// hist/first + 256*k
// counts = false: hist already holds the counts (an encoder launch with EncArgs::hist); only the
// first occurrences are computed
// the counted pipeline's first-occurrence pass (ie_huffman.hip first_scan_counted_kernel)
void launch_first_counted(const uint8_t* in, uint64_t pitch, const uint64_t* ends, uint64_t cap, int count,
                          uint32_t* hist, uint64_t* n, unsigned long long* first, unsigned* unresolved, uint32_t* h_hist,
                          unsigned long long* h_first, unsigned* h_unres, hipStream_t s);
void launch_first_full_batch(const uint8_t* in, uint64_t pitch, const uint64_t* n, uint64_t maxn, int count,
                             const uint32_t* hist, unsigned long long* first, const unsigned* unresolved, hipStream_t s);
void launch_hist_batch(const uint8_t* in, uint64_t pitch, const uint64_t* n, uint64_t maxn, int count, uint32_t* hist,
                       unsigned long long* first, unsigned* unresolved, hipStream_t s, bool counts = true);

struct DecArgs {
    int nframes, bx, by, rle;
    int add_base;            // P-frames: pixel = clamp(pixel already in out + (IDCT + 128)) (Block.cpp:110-119)
    uint8_t* out;
    uint64_t stride, frame_pitch;
    const EncTables* tab;
};

// Exact record parse + decode (ie_decode.hip): per-chunk transfer tables over every entry offset
// [0, D), composed per group of G tables (levels until at most G remain), then the decode with a
// look-back over record counts; no host round trip.  D = the longest record (4 + 15*(N*N+1) bits).
#ifndef IE_REC_M
#define IE_REC_M 1  // measured on 4K streams: 1 beats 2, 4 and 8 (occupancy over lane packing)
#endif
// tables per composition group: measured on 4K frames and the reference's example images, 32
// beats 64 and 128 (more workgroups and 32-step chases instead of 128: 4K 4x4 noise 186 -> 175-180
// us, 400x400 88 -> 81 us per decode; 16 is no faster)
#ifndef IE_REC_G4
#define IE_REC_G4 32
#endif
#ifndef IE_REC_G8
#define IE_REC_G8 32
#endif
template <int N> struct RecGeom {
    static constexpr int D = 4 + 15 * (N * N + 1);
    static constexpr int G = (N == 4) ? IE_REC_G4 : IE_REC_G8;  // tables per group ([G][D] 16-bit exits in LDS)
    static constexpr int M = IE_REC_M;              // chunks per table wave
    static constexpr int HSB = (N == 4) ? 10 : 11;  // claim hash slots per chunk: 1 << HSB
    static constexpr int HS = 1 << HSB;
};
constexpr int kRecMaxLevels = 6;  // G^6 chunks per decode call
constexpr int kRecPosCap = 256;  // record positions kept per chunk (more: the decode walks again)
constexpr int kRecWPB = 4;       // chunk waves per block of the per-chunk passes
#ifndef IE_DEC_CHUNKS
#define IE_DEC_CHUNKS 2
#endif
constexpr int kDecChunks = IE_DEC_CHUNKS;  // chunks per decode wave (about 32 records each)
struct RecParseArgs {
    const uint32_t* words;  // stream as stored (big-endian bytes), zero-padded by >= 2 words
    uint64_t nbits, start_bit;
    uint32_t C;             // chunk bits (multiple of 32)
    int nchunks, rle;
    uint16_t* tab;          // [nchunks][D] transfer tables (then prefix maps), followed by the
                            // composites of every level
    uint16_t* lvl[kRecMaxLevels];  // set by the launcher: the table array of every level
    int levels;
    uint32_t* E;            // [<= G] entry offset of every top-level composite
    uint64_t reserved0;     // unused: keeps the later members' offsets (profiles/decode_split_isa.txt)
    uint16_t* pos;          // [nchunks][kRecPosCap] record positions (relative to the chunk's word)
    uint32_t* cnt;          // [nchunks] records of every chunk
    uint32_t* lbase;        // [nchunks] records before every chunk within its count-pass workgroup
    uint32_t* wgsum;        // [count-pass workgroups] their record totals
    int seg;                // chunks per count-pass wave (rec_count_seg): a workgroup covers 4 * seg
    uint64_t* total;        // records on the true path
    uint64_t* end_out;      // end bit of the last block's record
    uint64_t reserved1;     // unused: as reserved0
    unsigned long long* wstamp; // diagnostics (IE_DEC_STAMPS): [table waves][8] phase times; nullptr = off
    int tm;                 // chunks per table wave (rec_table_geometry)
    int hbits;              // log2 of a table wave's claim slots
    // speculative parse (non-null): spec[k] = where the walk of chunk k from its first bit leaves
    // it (offset into chunk k+1) -- the entry of chunk k+1 in place of the composed tables; the
    // count pass, walking every chunk from its predecessor's spec exit, verifies each exit and sets
    // *fail on a mismatch (the decode pass then writes nothing and the host re-runs exactly)
    uint32_t* spec;
    unsigned* fail;         // device word, cleared by the speculative pass
    int warm;               // speculative walks start this many chunks early (IE_DEC_WARM, default 0)
    // device-chained span (ie_decode_gop): when non-null the first record is at
    // min(*dstart + start_add, nbits) -- an earlier launch's end bit -- and the span ends at most
    // `span` bits after it (start_bit is then unused); chunks past the span's end hold no record
    const uint64_t* dstart;
    uint64_t start_add, span;
    // image batch (ie_decode_images: the kernels' batch instantiations, blockIdx.y = the image; the
    // single-stream launches never read these).  Every image is a stream of its own from start_bit
    // with one chunk plan (C, nchunks: the longest stream's; a shorter stream's trailing chunks see
    // no stream bits and hold no record).  Image y reads words + y * img_words, is img_nbits[y] bits
    // long (nbits is then unused) and owns its scratch at the strides below; its total / end_out
    // are total[2 * y] / end_out[2 * y], its pixels DecArgs::out + y * frame_pitch (nframes = 1).
    const uint64_t* img_nbits;  // device [images]
    uint64_t img_words;         // 32-bit words between the images' streams
    uint64_t img_tab;           // 16-bit entries between the images' tab (and lvl[]) arrays
    uint32_t img_chunks;        // entries between the images' cnt / lbase (x kRecPosCap: pos)
    uint32_t img_wg;            // entries between the images' wgsum
    uint32_t img_E;             // entries between the images' E
};
// Table-wave geometry for chunks of C bits: chunks per wave (tm) and log2 claim slots (hbits).
void rec_table_geometry(uint32_t C, int n, int* tm, int* hbits);
int rec_group_chunks(int n);
int rec_entry_span(int n);
// Rows of D entries the parse of nchunks chunks needs in RecParseArgs::tab (the chunks' tables and
// every level's composites), and the composition levels over them (not capped at kRecMaxLevels).
size_t rec_table_rows(size_t nchunks, int n, int* levels);
size_t rec_decode_lds(uint32_t C, int n);
int rec_count_seg(uint32_t C);
// Returns the number of composition levels (< 0: too many chunks).
int launch_rec_parse_decode(RecParseArgs a, const DecArgs& d, int n, hipStream_t s);
// The same five passes over `images` independent streams (the img_ fields set; d.nframes = 1,
// image y's pixels at d.out + y * d.frame_pitch): every grid gains the image as its y dimension.
int launch_rec_parse_decode_images(RecParseArgs a, const DecArgs& d, int n, int images, hipStream_t s);
// The parse passes alone (tables, composition, counts), for a decode pass launched by the caller:
// fills a.tm, a.hbits and a.levels and returns the levels (< 0: too many chunks).  batch: the
// kernels' image-batch instantiations over `images` streams (else images is ignored).
int launch_rec_parse(RecParseArgs& a, int n, int images, bool batch, hipStream_t s);
// Region decode (ie_decode_region.hip): the same parse, then a decode pass that transforms only the
// blocks meeting the rectangle (x0, y0, rw, rh) of every frame (image) and stores only its pixels:
// pixel (x, y) of frame f at d.out + f * d.frame_pitch + (y - y0) * d.stride + (x - x0).  total and
// end_out are written as by the full decode.  d.add_base is not read.
int launch_rec_parse_decode_region(const RecParseArgs& a, const DecArgs& d, int n, int images, bool batch, int x0, int y0,
                                   int rw, int rh, hipStream_t s);
// Scaled decode (ie_decode_scaled.hip): the same parse, then a decode pass that transforms every
// block, takes the rounded integer mean of its pixels over scale x scale cells (scale = 1, 2, 4 or 8,
// at most n) and stores the (n/scale)^2 means: pixel (X, Y) of frame f's bx*n/scale x by*n/scale
// picture at d.out + f * d.frame_pitch + Y * d.stride + X.  total and end_out are written as by the
// full decode.  d.add_base is not read.  < -1: no such scale.
int launch_rec_parse_decode_scaled(const RecParseArgs& a, const DecArgs& d, int n, int images, bool batch, int scale,
                                   hipStream_t s);
// the speculative form (a.spec, a.fail set): speculative walks, verifying count pass, decode
void launch_rec_spec_decode(const RecParseArgs& a, const DecArgs& d, int n, hipStream_t s);

// Huffman decode (ie_huffman_decode.hip): write = false runs the exact parse (per-chunk transfer
// tables over the 15 entry offsets, composed) + the counting walk + scan and leaves the symbol
// count in *total (device); write = true then emits the symbols into out.  tab:
// huffman_table_rows() 16-bit words; E: at least 256 words.  Returns the composition levels (< 0
// on error).
int huffman_decode_device(const uint32_t* W, uint64_t nbits, uint64_t start_bit, const uint16_t* lut,
                          uint64_t chunk_bits, uint64_t* entry, uint16_t* tab, uint32_t* E, uint32_t* count,
                          uint64_t* base, unsigned* changed, uint64_t* total, uint8_t* out, bool write, hipStream_t s,
                          uint64_t out_cap = ~0ull);
size_t huffman_table_rows(uint64_t nbits, uint64_t start_bit, uint64_t chunk_bits);

// The same decode for `images` streams side by side in one set of launches (the kernels' batch
// instantiations: blockIdx.y = the image).  One chunk plan: nchunks chunks of chunk_bits for every
// image, from the longest code stream; an image's chunks past its stream hold no code.  Every
// array holds the images' parts one after another: image k's at k times the stride given.
struct HufBatch {
    int images, nchunks;
    uint64_t chunk_bits;
    const uint32_t* words;      // image k's stream: words + k * img_words
    size_t img_words;
    const uint64_t* nbits;      // [images] (device) stream bits
    const uint64_t* start_bit;  // [images] (device) first bit of the code stream
    const uint16_t* lut;        // [images][32768] prefix tables
    uint16_t* tab;              // [images][huffman_batch_tab(nchunks)]
    uint64_t* entry;            // [images][nchunks]
    uint64_t* base;             // [images][nchunks]
    uint32_t* count;            // [images][nchunks]
    uint32_t* wgsum;            // [images][huffman_batch_wg(nchunks)]
    uint32_t* E;                // [images][huffman_batch_entries()]
    unsigned* flags;            // [images][2], zero before the launches: [0] symbols past out_pitch
                                // (not written), [1] a bit string no code prefixes
    uint64_t* total;            // [images] symbol counts
    uint8_t* out;               // write: image k's symbols at out + k * out_pitch, at most out_pitch
    size_t out_pitch;
};
size_t huffman_batch_tab(int nchunks);  // 16-bit table entries per image (a multiple of 8)
uint32_t huffman_batch_wg(int nchunks);
uint32_t huffman_batch_entries();
// write = false: table pass, composition, counts, totals (returns the composition levels, < 0 on
// error); write = true: the emit.
int huffman_decode_images(const HufBatch& b, bool write, hipStream_t s);

// P-frame of a gop > 1 video (ie_pframe.hip): one launch sequence per frame, chained on the device.
struct PfArgs {
    const uint8_t* cur;      // the frame, rows cs apart
    uint64_t cs;
    const uint8_t* ref;      // the previous frame's buffer as the reference leaves it, rows rs apart
    uint64_t rs;
    uint8_t* rec;            // [h][w]: this frame's buffer after the P-frame pass (the next reference)
    int w, h, mbx, mby, bx;  // macroblocks per row / column (floor), microblocks per row
    int rle, merange, mv_bits;
    const EncTables* tab;
    int16_t* coef;           // [bx*by][16] quantised prediction error (natural order), 4x4 only
    uint32_t* bits;          // [bx*by] record bits, 0 = no record
    uint32_t* out;           // stream words (zero from the frame's first bit on)
    const uint64_t* start;   // device: the frame's first bit
    uint64_t* end;           // device: its end bit
    uint64_t* st;            // record tiles' chain state (look-back scan); nullptr = separate scan launches
    uint32_t tag;            // the state's epoch
    unsigned* err;           // [0]: look-back spin timeouts
    // Group batch (launch_pframe_groups: blockIdx.y = the group).  Group g's frame, reference,
    // buffer, coefficients, record lengths, tile sums and output slot lie g times these strides (in
    // elements of each array) past the pointers above, its first / end bit in start[g] / end[g].
    // All 0 with one group: the single-frame launch.
    uint64_t g_cur, g_ref, g_rec, g_coef, g_bits, g_tile, g_out;
};
void launch_pframe(const PfArgs& a, int n, uint64_t* tile_scratch, hipStream_t s);
// The same P-frame of `groups` independent groups of pictures in one set of launches (the g_
// strides set, a.st ignored): macroblocks, then tile sums / tile scan / emission in every mode --
// no look-back chain per group.  groups <= 65535 (grid.y).
void launch_pframe_groups(const PfArgs& a, int n, int groups, uint64_t* tile_scratch, hipStream_t s);

// ie_probe_gop (ie_pframe.hip): one P-frame step of `groups` groups of pictures under nm candidate
// matrices, sizes only.  blockIdx.y = the group, blockIdx.z = a range of mper candidates.
struct PgArgs {
    const uint8_t* cur;      // group 0's frame of this step, rows cs apart; group g's: + g * g_cur
    uint64_t cs, g_cur;
    // Candidate m of group g predicts from ref + g * g_ref + m * m_ref, rows rs apart.  m_ref == 0:
    // one reference for all candidates (a group's first P-frame: the I-frame's source) -- search
    // and unquantised coefficients are then formed once per macroblock.
    const uint8_t* ref;
    uint64_t rs, g_ref, m_ref;
    // its reconstruction: rec + g * g_rec + m * m_rec, [h][w]; nullptr: not stored (no later step reads it)
    uint8_t* rec;
    uint64_t g_rec, m_rec;
    int w, h, mbx, mby;
    int rle, merange, mv_bits;
    const EncTables* tab;    // P, R and S (they do not depend on the matrix)
    const uint16_t* q;       // [nm][16] the candidates in ZIG-ZAG order (device)
    int nm, mper;            // candidates of the launch (m = 0 .. nm-1), candidates per wave (1 .. 64)
    // 2 * mv_bits + the record bits of every macroblock are added to bits[m * m_bits + g * g_bits]
    unsigned long long* bits;
    uint64_t m_bits, g_bits;
};
void launch_pframe_probe(const PgArgs& a, int groups, hipStream_t s);
// ie_probe_gop_rd: the same step carrying the decoder's frame chain next to the encoder's.  W and
// H are multiples of 16 (no uncovered strips).  Candidate m of group g copies its blocks from its
// own DECODED previous frame, dref + g * g_dec + m * m_dec, and leaves this frame's decoded pixels
// in dec + g * g_dec + m * m_dec (both [h][w]; dec == nullptr: not stored); the squared error
// against cur is added to sse[m * m_bits + g * g_bits].  bits may be nullptr here.
struct PgRdArgs : PgArgs {
    const uint8_t* dref;
    uint8_t* dec;
    uint64_t g_dec, m_dec;
    int motioncomp;          // 0: the decoder copies the blocks and drops the error
    unsigned long long* sse;
};
void launch_pframe_probe_rd(const PgRdArgs& a, int groups, hipStream_t s);
// dst[m * nframes + g * gop] = src[m * groups + g] (the I-frames' sums); fill: every other entry = pconst
void launch_pframe_probe_scatter(const unsigned long long* src, unsigned long long* dst, int nq, int nframes, int gop,
                                 int groups, int fill, unsigned long long pconst, hipStream_t s);

// Splice of a video's groups of pictures (ie_encode_gop_groups): group g's private slot (bits
// [0, len_g) from slots + g * slot_words) goes to out at bit base + sum_{k<g} len_k.
struct GopSplice {
    const uint64_t* pos;     // [gop + 1][groups]: pos[j * groups + g] = first bit of group g's frame j in its slot
    int groups, gop, nframes;  // of this wave; nframes <= groups * gop (only the last group can be short)
    const uint32_t* slots;
    uint64_t slot_words;
    uint32_t* out;           // zero from the base bit on
    uint64_t base;           // the wave's first bit in out ...
    const uint64_t* base_dev;  // ... or, when non-null, *base_dev (the previous wave's end bit)
    uint64_t* goff;          // [groups + 1] scratch: every group's first bit in out, then the wave's end
    uint64_t* fpos;          // [nframes + 1]: every frame's first bit in out, then the wave's end
};
void launch_gop_splice(const GopSplice& a, hipStream_t s);
// P-frame decode, first half (Block.cpp:481-496): every macroblock's motion vector read from the
// stream words (big-endian bytes) at start_bit, the previous decoded frame's block at the clamped
// vector copied into place
// gop decode: pos[0] = start, pos[1..n] = ~0 (no end yet), tot[0..n) = 0
void launch_gop_init(uint64_t* pos, uint64_t* tot, int n, uint64_t start, hipStream_t s);
// the same arrays with pos[0] = *prev_end (device: the end word of the chunk of frames before)
void launch_gop_continue(uint64_t* pos, uint64_t* tot, int n, const uint64_t* prev_end, hipStream_t s);
// dstart non-null: the vectors start at *dstart (device, an earlier launch's end bit) in place of
// start_bit; a macroblock whose vector lies past nbits copies nothing (the caller reports it)
void launch_pframe_mvcopy(const uint8_t* stream, uint64_t start_bit, const uint64_t* dstart, uint64_t nbits, int mv_bits,
                          const uint8_t* ref, uint64_t rs, uint8_t* out, uint64_t os, int w, int h, hipStream_t s);
int pframe_tiles(int nb);    // tile_scratch entries

}  // namespace ie
