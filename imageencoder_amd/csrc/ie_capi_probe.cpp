// imageencoder_amd/csrc/ie_capi_probe.cpp -- ie_probe_sizes: the payload bits of a batch of frames
// under many candidate quantisation matrices, from one pass over the pixels (ie_probe.hip), and
// ie_probe_rd: the squared error of the decoded pixels as well.  They read the context's P / S / R
// tables (they depend on the block size only) and leave its matrix, tables, chain state and end
// bits alone.
#include "ie_ctx.hpp"

using namespace iec;

namespace {
// algo.cpp:68-87: natural index of zig-zag position z (the kernel's lanes are zig-zag positions)
const uint8_t kZz4[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
const uint8_t kZz8[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

}  // namespace

namespace iec {

int check_candidates(ie_ctx* c, const uint16_t* q, int nq) {
    if (nq < 1 || nq > IE_PROBE_MAX)
        return fail(c, IE_EINVAL, "nq must be in [1, " + std::to_string(int(IE_PROBE_MAX)) + "]");
    const int nn = c->n * c->n;
    for (int m = 0; m < nq; m++)
        for (int k = 0; k < nn; k++)
            if (q[size_t(m) * nn + k] == 0)
                return fail(c, IE_EINVAL, "candidate matrix " + std::to_string(m) + " has a zero entry (entries must be > 0)");
    return IE_OK;
}

// (an earlier call's copy out of the pinned block may still be in flight when the calls are
// asynchronous: the event after it is waited for before the block is written again)
int stage_candidates(ie_ctx* c, const uint16_t* q, int nq) {
    const int n = c->n, nn = n * n;
    const size_t qcap = size_t(IE_PROBE_MAX) * 64;
    int r;
    if ((r = c->h_probe_q.reserve(c, qcap))) return r;
    if ((r = c->d_probe_q.reserve(c, qcap))) return r;
    if ((r = c->ev_probe.create(c, hipEventDisableTiming))) return r;
    if (c->probe_recorded) HIPCHK(c, hipEventSynchronize(c->ev_probe));
    const uint8_t* zz = n == 4 ? kZz4 : kZz8;
    for (int m = 0; m < nq; m++)
        for (int z = 0; z < nn; z++) c->h_probe_q[size_t(m) * nn + z] = q[size_t(m) * nn + zz[z]];
    HIPCHK(c, hipMemcpyAsync(c->d_probe_q, c->h_probe_q, size_t(nq) * nn * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_probe, c->stream));
    c->probe_recorded = true;
    return IE_OK;
}

}  // namespace iec

namespace {
// Both entry points.  sse == nullptr: ie_probe_sizes (bits required); else ie_probe_rd (bits optional).
int probe(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes, int use_rle,
          const uint16_t* q, int nq, uint64_t* bits, uint64_t* sse, bool rd) {
    if (!c || !y || !q || (rd ? !sse : !bits)) return IE_EINVAL;
    int r = check_frames(c, w, h, nframes, stride, frame_pitch);
    if (r) return r;
    if ((r = check_candidates(c, q, nq))) return r;
    const int n = c->n;
    HIPCHK(c, hipSetDevice(c->device));
    const bool in_dev = is_device_ptr(y);
    const bool res_dev = is_device_ptr(rd ? sse : bits);
    if (rd && bits && is_device_ptr(bits) != res_dev)
        return fail(c, IE_EINVAL, "bits and sse must be both host or both device memory");
    if (res_dev && bits && reinterpret_cast<uintptr_t>(bits) % 8) return fail(c, IE_EINVAL, "device bits must be 8-byte aligned");
    if (res_dev && rd && reinterpret_cast<uintptr_t>(sse) % 8) return fail(c, IE_EINVAL, "device sse must be 8-byte aligned");

    const uint8_t* dy;
    if ((r = stage_in(c, y, in_dev, frames_span(nframes, frame_pitch, stride, w, h), &dy))) return r;

    if ((r = stage_candidates(c, q, nq))) return r;

    // host results: the sums (ie_probe_rd: the bits, then the squared errors) in one device block
    const size_t nsums = size_t(nq) * size_t(nframes);
    uint64_t *dbits = bits, *dsse = sse;
    if (!res_dev) {
        if ((r = c->d_probe_bits.reserve(c, nsums * (rd ? 2 : 1)))) return r;
        dbits = c->d_probe_bits;
        dsse = rd ? dbits + nsums : nullptr;
        if (rd && (r = c->h_probe_out.reserve(c, nsums * 2))) return r;
        HIPCHK(c, hipMemsetAsync(dbits, 0, nsums * (rd ? 2 : 1) * sizeof(uint64_t), c->stream));
    } else {
        if (dbits) HIPCHK(c, hipMemsetAsync(dbits, 0, nsums * sizeof(uint64_t), c->stream));
        if (rd) HIPCHK(c, hipMemsetAsync(dsse, 0, nsums * sizeof(uint64_t), c->stream));
    }

    ie::ProbeArgs a{};
    a.y = dy;
    a.stride = stride;
    a.frame_pitch = frame_pitch;
    a.bx = w / n;
    a.by = h / n;
    a.nframes = nframes;
    a.rle = use_rle ? 1 : 0;
    a.vec_ok = (reinterpret_cast<uintptr_t>(dy) % 4 == 0 && stride % 4 == 0 && (nframes == 1 || frame_pitch % 4 == 0)) ? 1 : 0;
    a.nq = nq;
    a.q = c->d_probe_q;
    a.tab = c->d_tab;
    a.bits = reinterpret_cast<unsigned long long*>(dbits);
    if (rd)
        ie::launch_probe_rd(a, reinterpret_cast<unsigned long long*>(dsse), n, c->stream);
    else
        ie::launch_probe_sizes(a, n, c->stream);
    HIPCHK(c, hipGetLastError());
    if (res_dev) return IE_OK;  // asynchronous on the context's stream
    if (!rd) {
        HIPCHK(c, hipMemcpyAsync(bits, dbits, nsums * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return IE_OK;
    }
    // one read-back for both arrays, through pinned memory
    HIPCHK(c, hipMemcpyAsync(c->h_probe_out, dbits, nsums * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bits) std::copy(c->h_probe_out + 0, c->h_probe_out + nsums, bits);
    std::copy(c->h_probe_out + nsums, c->h_probe_out + 2 * nsums, sse);
    return IE_OK;
}
}  // namespace

extern "C" int ie_probe_sizes(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                              int use_rle, const uint16_t* q, int nq, uint64_t* bits) {
    return probe(c, y, w, h, stride, frame_pitch, nframes, use_rle, q, nq, bits, nullptr, false);
}

extern "C" int ie_probe_rd(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                           int use_rle, const uint16_t* q, int nq, uint64_t* bits, uint64_t* sse) {
    return probe(c, y, w, h, stride, frame_pitch, nframes, use_rle, q, nq, bits, sse, true);
}
