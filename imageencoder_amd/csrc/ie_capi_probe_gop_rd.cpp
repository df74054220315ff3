// imageencoder_amd/csrc/ie_capi_probe_gop_rd.cpp -- ie_probe_gop_rd: ie_probe_gop's table, and with
// it the squared error of the pixels ie_decode_gop would write for every frame under every
// candidate matrix, without writing or parsing a stream.
//
// The decoder's frames are a chain of their own next to the encoder's reconstructions: a group's
// decoder starts from the LOSSY decoded I-frame (the encoder's first P-frame predicts from the
// I-frame's source), copies its blocks at the vector as the stream holds it and adds the error as
// the record holds it.  So every (group, candidate) pair of a wave owns four frames of scratch --
// two encoder reconstructions and two decoded frames, each pair alternating -- in a buffer of its
// own (d_probe_gop_rd).  Per wave: probe_kernel<4, true, true> over the wave's I-frames (bits,
// squared error, and the decoded pixels stored into the pairs' first decoded frame), then
// pf_probe_kernel<PgRdArgs> per step j = 1 .. gop-1.  Like the other probes it reads the context's
// P / S / R tables and leaves its matrix, tables, chain state, end bits, the encoders' gop scratch
// and ie_probe_gop's scratch alone.
#include "ie_ctx.hpp"

using namespace iec;

extern "C" int ie_probe_gop_rd(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                               int gop, int merange, int use_rle, int motioncomp, const uint16_t* q, int nq,
                               uint64_t* bits, uint64_t* sse) {
    if (!c || !y || !q || !sse) return IE_EINVAL;
    gop = std::max(1, gop);
    size_t need = 0;
    int r = check_gop(c, w, h, stride, frame_pitch, nframes, gop, merange, SIZE_MAX, 0, &need);
    if (r) return r;
    if ((r = check_candidates(c, q, nq))) return r;
    const bool pframes = gop > 1 && nframes > 1;
    if (pframes && (w % 16 || h % 16))  // ie_decode_gop's rule: no decoded pixels exist to compare with
        return fail(c, IE_EINVAL, "P-frames decode for W and H multiples of 16 only: there is no decoded video to measure");
    if (!pframes) return ie_probe_rd(c, y, w, h, stride, frame_pitch, nframes, use_rle, q, nq, bits, sse);
    const int n = c->n;
    if (n != 4)
        // ie_encode_gop writes no microblock records for 8x8 P-frames, ie_decode_gop reads one per
        // microblock: it parses the following frames' bits as records, or runs out of stream
        return fail(c, IE_EINVAL, "8x8 P-frame streams do not decode (the encoder writes no records, the decoder reads "
                                  "one per block): there is no decoded video to measure");
    HIPCHK(c, hipSetDevice(c->device));
    const bool in_dev = is_device_ptr(y), res_dev = is_device_ptr(sse);
    if (bits && is_device_ptr(bits) != res_dev) return fail(c, IE_EINVAL, "bits and sse must be both host or both device memory");
    if (res_dev && bits && reinterpret_cast<uintptr_t>(bits) % 8) return fail(c, IE_EINVAL, "device bits must be 8-byte aligned");
    if (res_dev && reinterpret_cast<uintptr_t>(sse) % 8) return fail(c, IE_EINVAL, "device sse must be 8-byte aligned");
    const uint8_t* dy;
    if ((r = stage_in(c, y, in_dev, frames_span(nframes, frame_pitch, stride, w, h), &dy))) return r;
    if ((r = stage_candidates(c, q, nq))) return r;

    // host results: the bits, then the squared errors, in one device block read back together
    const size_t nsums = size_t(nq) * size_t(nframes);
    uint64_t *dbits = bits, *dsse = sse;
    if (!res_dev) {
        if ((r = c->d_probe_bits.reserve(c, 2 * nsums))) return r;
        if ((r = c->h_probe_out.reserve(c, 2 * nsums))) return r;
        dbits = c->d_probe_bits;
        dsse = dbits + nsums;
        HIPCHK(c, hipMemsetAsync(dbits, 0, 2 * nsums * sizeof(uint64_t), c->stream));
    } else {
        if (dbits) HIPCHK(c, hipMemsetAsync(dbits, 0, nsums * sizeof(uint64_t), c->stream));
        HIPCHK(c, hipMemsetAsync(dsse, 0, nsums * sizeof(uint64_t), c->stream));
    }
    unsigned long long* const ubits = reinterpret_cast<unsigned long long*>(dbits);
    unsigned long long* const usse = reinterpret_cast<unsigned long long*>(dsse);

    // Waves, as ie_probe_gop: at most `pairs` (group, candidate) pairs hold scratch at a time, four
    // frames each -- what keeps it under 1 GiB, lowered further by IE_PROBE_GOP_MAX (read on every
    // call).  Whole groups with all candidates while that many fit; otherwise one group at a time,
    // chunks of candidates.
    const int G = (nframes + gop - 1) / gop, Gp = (nframes - 1 + gop - 1) / gop;  // groups; those with a P-frame
    const int mbx = w / 16, mby = h / 16, mv = mvec_bits(merange);
    const size_t fpx = size_t(w) * h, pair_bytes = 4 * fpx, group_pitch = size_t(gop) * frame_pitch;
    size_t pairs = std::max<size_t>(1, (size_t(1) << 30) / pair_bytes);
    if (const char* eb = getenv("IE_PROBE_GOP_MAX"))
        if (atoll(eb) > 0) pairs = std::min<size_t>(pairs, size_t(atoll(eb)));
    const int chunk = int(std::min<size_t>(pairs, size_t(nq)));
    const int Gw = chunk < nq ? 1 : int(std::min<size_t>({size_t(Gp), pairs / size_t(nq), size_t(65535)}));
    if ((r = c->d_probe_gop_rd.reserve(c, size_t(Gw) * size_t(chunk) * pair_bytes))) return r;
    uint8_t* const rec = c->d_probe_gop_rd;  // a pair: reconstruction 0, 1, decoded frame 0, 1
    uint8_t* const dec = rec + 2 * fpx;

    // the I-frames of `ng` groups from frame f0 under candidates [m0, m0 + nm); the first `store`
    // of them leave their decoded pixels in their pairs' decoded frame 0
    const auto iframes = [&](int f0, int ng, int m0, int nm, int store) {
        ie::ProbeArgs ia{};
        ia.y = dy + size_t(f0) * frame_pitch;
        ia.stride = stride;
        ia.frame_pitch = group_pitch;
        ia.bx = w / n;
        ia.by = h / n;
        ia.nframes = ng;
        ia.rle = use_rle ? 1 : 0;
        ia.vec_ok = (reinterpret_cast<uintptr_t>(dy) % 4 == 0 && stride % 4 == 0 && frame_pitch % 4 == 0) ? 1 : 0;
        ia.nq = nm;
        ia.q = c->d_probe_q + size_t(m0) * 16;
        ia.tab = c->d_tab;
        ia.bits = ubits ? ubits + size_t(m0) * size_t(nframes) + size_t(f0) : nullptr;
        ia.out_m = uint64_t(nframes);
        ia.out_f = uint64_t(gop);
        ia.dec = dec;
        ia.f_dec = size_t(chunk) * pair_bytes;
        ia.m_dec = pair_bytes;
        ia.dec_frames = store;
        ie::launch_probe_rd_store(ia, usse + size_t(m0) * size_t(nframes) + size_t(f0), c->stream);
    };

    for (int g0 = 0; g0 < Gp; g0 += Gw) {
        const int gw = std::min(Gw, Gp - g0);
        const int f0 = g0 * gop;
        const int nfw = int(std::min<int64_t>(int64_t(nframes) - f0, int64_t(gw) * gop));
        const int steps = std::min(gop, nfw);  // frames of the wave's longest group
        for (int m0 = 0; m0 < nq; m0 += chunk) {
            const int nm = std::min(chunk, nq - m0);
            iframes(f0, gw, m0, nm, gw);
            HIPCHK(c, hipGetLastError());
            for (int j = 1; j < steps; j++) {
                ie::PgRdArgs a{};
                a.cur = dy + size_t(f0 + j) * frame_pitch;
                a.cs = stride;
                a.g_cur = group_pitch;
                a.g_rec = a.g_dec = size_t(chunk) * pair_bytes;
                a.m_rec = a.m_dec = pair_bytes;
                if (j == 1) {  // the encoder predicts from the I-frame as the caller holds it, shared by the candidates
                    a.ref = dy + size_t(f0) * frame_pitch;
                    a.rs = stride;
                    a.g_ref = group_pitch;
                    a.m_ref = 0;
                } else {       // and from then on from every candidate's own reconstruction
                    a.ref = rec + size_t((j - 1) & 1) * fpx;
                    a.rs = size_t(w);
                    a.g_ref = a.g_rec;
                    a.m_ref = a.m_rec;
                }
                a.dref = dec + size_t((j - 1) & 1) * fpx;  // the decoder never shares: frame 0 is the decoded I-frame
                const bool last = j + 1 >= steps;          // nothing reads the last step's frames
                a.rec = last ? nullptr : rec + size_t(j & 1) * fpx;
                a.dec = last ? nullptr : dec + size_t(j & 1) * fpx;
                a.w = w;
                a.h = h;
                a.mbx = mbx;
                a.mby = mby;
                a.rle = use_rle ? 1 : 0;
                a.merange = merange;
                a.mv_bits = mv;
                a.motioncomp = motioncomp ? 1 : 0;
                a.tab = c->d_tab;
                a.q = c->d_probe_q + size_t(m0) * 16;
                a.nm = nm;
                a.mper = j == 1 ? nm : 1;  // a shared reference: the candidates loop inside the wave
                const size_t at = size_t(m0) * size_t(nframes) + size_t(f0 + j);
                a.bits = ubits ? ubits + at : nullptr;
                a.sse = usse + at;
                a.m_bits = uint64_t(nframes);
                a.g_bits = uint64_t(gop);
                const int gj = std::min(gw, (nfw - j + gop - 1) / gop);  // the groups that have a frame j
                ie::launch_pframe_probe_rd(a, gj, c->stream);
                HIPCHK(c, hipGetLastError());
            }
        }
    }
    if (G > Gp) {  // a last group of one I-frame: nothing follows it, nothing is stored
        iframes(Gp * gop, 1, 0, nq, 0);
        HIPCHK(c, hipGetLastError());
    }
    if (res_dev) return IE_OK;  // asynchronous on the context's stream
    HIPCHK(c, hipMemcpyAsync(c->h_probe_out, dbits, 2 * nsums * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (bits) std::copy(c->h_probe_out + 0, c->h_probe_out + nsums, bits);
    std::copy(c->h_probe_out + nsums, c->h_probe_out + 2 * nsums, sse);
    return IE_OK;
}
