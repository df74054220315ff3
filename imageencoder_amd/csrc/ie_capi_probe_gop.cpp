// imageencoder_amd/csrc/ie_capi_probe_gop.cpp -- ie_probe_gop: the payload bits of every frame of a
// video with P-frames under many candidate quantisation matrices, without writing a stream.
//
// I-frames: ie_probe_sizes' kernel over the I-frames alone (they are gop frames apart), scattered
// into the table.  P-frames with 4x4 blocks: pf_probe_kernel (ie_pframe.hip), one set of launches
// per step j = 1 .. gop-1 over all groups that have such a frame, every (group, candidate) pair
// with two reconstructed frames of its own.  P-frames with 8x8 blocks carry vectors only
// (ImageBase.cpp:271): their size is a constant and no macroblock kernel runs.  Like the other
// probes it reads the context's P / S / R tables and leaves its matrix, tables, chain state, end
// bits and the encoders' gop scratch alone.
#include "ie_ctx.hpp"

using namespace iec;

extern "C" int ie_probe_gop(ie_ctx* c, const uint8_t* y, int w, int h, size_t stride, size_t frame_pitch, int nframes,
                            int gop, int merange, int use_rle, const uint16_t* q, int nq, uint64_t* bits) {
    if (!c || !y || !q || !bits) return IE_EINVAL;
    gop = std::max(1, gop);
    size_t need = 0;
    int r = check_gop(c, w, h, stride, frame_pitch, nframes, gop, merange, SIZE_MAX, 0, &need);
    if (r) return r;
    if ((r = check_candidates(c, q, nq))) return r;
    if (gop <= 1 || nframes == 1)  // no P-frame
        return ie_probe_sizes(c, y, w, h, stride, frame_pitch, nframes, use_rle, q, nq, bits);
    HIPCHK(c, hipSetDevice(c->device));
    const bool in_dev = is_device_ptr(y), res_dev = is_device_ptr(bits);
    if (res_dev && reinterpret_cast<uintptr_t>(bits) % 8) return fail(c, IE_EINVAL, "device bits must be 8-byte aligned");
    const uint8_t* dy;
    if ((r = stage_in(c, y, in_dev, frames_span(nframes, frame_pitch, stride, w, h), &dy))) return r;
    if ((r = stage_candidates(c, q, nq))) return r;

    // the table (host results: in d_probe_bits), then the I-frames' sums [nq][G]
    const int n = c->n, G = (nframes + gop - 1) / gop;
    const size_t nsums = size_t(nq) * size_t(nframes), nisums = size_t(nq) * size_t(G);
    if ((r = c->d_probe_bits.reserve(c, (res_dev ? 0 : nsums) + nisums))) return r;
    uint64_t* dbits = res_dev ? bits : c->d_probe_bits.get();
    uint64_t* disum = c->d_probe_bits + (res_dev ? 0 : nsums);
    HIPCHK(c, hipMemsetAsync(dbits, 0, nsums * sizeof(uint64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(disum, 0, nisums * sizeof(uint64_t), c->stream));

    const size_t group_pitch = size_t(gop) * frame_pitch;
    ie::ProbeArgs ia{};
    ia.y = dy;
    ia.stride = stride;
    ia.frame_pitch = group_pitch;
    ia.bx = w / n;
    ia.by = h / n;
    ia.nframes = G;
    ia.rle = use_rle ? 1 : 0;
    ia.vec_ok = (reinterpret_cast<uintptr_t>(dy) % 4 == 0 && stride % 4 == 0 && group_pitch % 4 == 0) ? 1 : 0;
    ia.nq = nq;
    ia.q = c->d_probe_q;
    ia.tab = c->d_tab;
    ia.bits = reinterpret_cast<unsigned long long*>(disum);
    ie::launch_probe_sizes(ia, n, c->stream);
    HIPCHK(c, hipGetLastError());

    // P-frames whose size is a closed form: the vectors of the macroblocks and nothing else
    const int mbx = w / 16, mby = h / 16, nmb = mbx * mby, mv = mvec_bits(merange);
    const bool closed = n != 4 || nmb == 0;
    ie::launch_pframe_probe_scatter(reinterpret_cast<const unsigned long long*>(disum),
                                    reinterpret_cast<unsigned long long*>(dbits), nq, nframes, gop, G, closed ? 1 : 0,
                                    uint64_t(nmb) * 2u * uint64_t(mv), c->stream);
    HIPCHK(c, hipGetLastError());

    if (!closed) {
        // Waves: at most `pairs` (group, candidate) pairs hold scratch at a time -- what keeps it
        // under 1 GiB, lowered further by IE_PROBE_GOP_MAX (read on every call).  Whole groups with
        // all candidates while that many fit; otherwise one group at a time, chunks of candidates.
        const size_t fpx = size_t(w) * h, pair_bytes = 2 * fpx;
        size_t pairs = std::max<size_t>(1, (size_t(1) << 30) / pair_bytes);
        if (const char* eb = getenv("IE_PROBE_GOP_MAX"))
            if (atoll(eb) > 0) pairs = std::min<size_t>(pairs, size_t(atoll(eb)));
        const int Gp = (nframes - 1 + gop - 1) / gop;  // groups with a P-frame
        const int chunk = int(std::min<size_t>(pairs, size_t(nq)));
        const int Gw = chunk < nq ? 1 : int(std::min<size_t>({size_t(Gp), pairs / size_t(nq), size_t(65535)}));
        if ((r = c->d_probe_gop.reserve(c, size_t(Gw) * size_t(chunk) * pair_bytes))) return r;
        for (int g0 = 0; g0 < Gp; g0 += Gw) {
            const int gw = std::min(Gw, Gp - g0);
            const int f0 = g0 * gop;
            const int nfw = int(std::min<int64_t>(int64_t(nframes) - f0, int64_t(gw) * gop));
            const int steps = std::min(gop, nfw);  // frames of the wave's longest group
            for (int m0 = 0; m0 < nq; m0 += chunk) {
                const int nm = std::min(chunk, nq - m0);
                for (int j = 1; j < steps; j++) {
                    ie::PgArgs a{};
                    a.cur = dy + size_t(f0 + j) * frame_pitch;
                    a.cs = stride;
                    a.g_cur = group_pitch;
                    a.g_rec = size_t(chunk) * pair_bytes;
                    a.m_rec = pair_bytes;
                    if (j == 1) {  // the I-frame as the caller holds it, shared by the candidates
                        a.ref = dy + size_t(f0) * frame_pitch;
                        a.rs = stride;
                        a.g_ref = group_pitch;
                        a.m_ref = 0;
                    } else {       // every candidate's own reconstruction of the previous P-frame
                        a.ref = c->d_probe_gop + size_t((j - 1) & 1) * fpx;
                        a.rs = size_t(w);
                        a.g_ref = a.g_rec;
                        a.m_ref = a.m_rec;
                    }
                    a.rec = j + 1 < steps ? c->d_probe_gop + size_t(j & 1) * fpx : nullptr;
                    a.w = w;
                    a.h = h;
                    a.mbx = mbx;
                    a.mby = mby;
                    a.rle = use_rle ? 1 : 0;
                    a.merange = merange;
                    a.mv_bits = mv;
                    a.tab = c->d_tab;
                    a.q = c->d_probe_q + size_t(m0) * 16;
                    a.nm = nm;
                    a.mper = j == 1 ? nm : 1;  // a shared reference: the candidates loop inside the wave
                    a.bits = reinterpret_cast<unsigned long long*>(dbits) + size_t(m0) * size_t(nframes) + size_t(f0 + j);
                    a.m_bits = uint64_t(nframes);
                    a.g_bits = uint64_t(gop);
                    const int gj = std::min(gw, (nfw - j + gop - 1) / gop);  // the groups that have a frame j
                    ie::launch_pframe_probe(a, gj, c->stream);
                    HIPCHK(c, hipGetLastError());
                }
            }
        }
    }
    if (res_dev) return IE_OK;  // asynchronous on the context's stream
    HIPCHK(c, hipMemcpyAsync(bits, dbits, nsums * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return IE_OK;
}
