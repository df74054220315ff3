// imageencoder_amd/csrc/ie_capi.cpp -- the extern "C" boundary (include/ie_hip.h), part 1: the
// context and what every other part shares (ie_ctx.hpp), quantisation tables, memory calls.  The
// encoders are in ie_capi_encode.cpp and ie_capi_stream.cpp, the Huffman calls in
// ie_capi_huffman.cpp, the decoders in ie_capi_decode.cpp.  Host code; compiled with hipcc.
#include "ie_ctx.hpp"

using namespace iec;

namespace iec {

int prepare_state(ie_ctx* c, int ntiles, int nframes) {
    int r;
    if (size_t(ntiles) > c->state_tiles()) {
        // the tile capacity doubles; d_wave_fix is sized from it (the stream has been waited for by then)
        const size_t cap = std::max<size_t>(ntiles, c->state_tiles() * 2);
        if ((r = c->d_state.reserve(c, size_t(ie::kStateWordsPerTile) * cap))) return r;
        if ((r = c->d_wave_fix.reserve(c, cap * 16, Wait::None))) return r;
        HIPCHK(c, hipMemsetAsync(c->d_state, 0, c->d_state.cap() * sizeof(uint64_t), c->stream));
        c->tag = 0;
    }
    c->tag++;
    if (c->tag > 255) {
        HIPCHK(c, hipMemsetAsync(c->d_state, 0, c->d_state.cap() * sizeof(uint64_t), c->stream));
        c->tag = 1;
    }
    // at least 64 frames; the two grow together
    const size_t frames = std::max<size_t>(nframes, 64);
    if ((r = c->d_frame_start.reserve(c, frames))) return r;
    return c->d_chain_end.reserve(c, frames, Wait::None);
}

// Timing marks around the batched Huffman stages (ie_last_stage_ms): event i on the context's stream.
int stage_mark(ie_ctx* c, int i) {
    if (!c->stage_timing) return IE_OK;  // (ie_set_stage_timing: off by default)
    if (int r = c->stage_ev[i].create(c)) return r;
    HIPCHK(c, hipEventRecord(c->stage_ev[i], c->stream));
    if (i & 1) c->stage_rec[i >> 1] = true;
    return IE_OK;
}

static const char kTimedOut[] = "tile look-back timed out";
int lookback_failed(ie_ctx* c, const char* where) { return fail(c, IE_EDEVICE, std::string(kTimedOut) + where); }

int ticket_redo(ie_ctx* c, unsigned timeouts, bool* redo) {
    *redo = false;
    if (!timeouts) return IE_OK;
    if (c->use_ticket) return lookback_failed(c);
    c->use_ticket = *redo = true;
    return IE_OK;
}

// d_err ([0] look-back timeouts; sum of [2..65] = FP64 re-evaluations).  Synchronises the stream.
// The device counters only ever grow (no per-launch reset kernel in the launch path); a read
// reports the increments since the previous read.
int read_errors(ie_ctx* c, unsigned* timeouts, uint64_t* fallbacks) {
    unsigned e[kErrWords];
    HIPCHK(c, hipMemcpyAsync(e, c->d_err, sizeof(e), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t f = 0;
    if (fallbacks && c->last_fix_words) {
        std::vector<uint32_t> w(size_t(c->last_fix_words));
        HIPCHK(c, hipMemcpy(w.data(), c->d_wave_fix, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t v : w) f += v;
    }
    unsigned t = e[0] - c->err_seen[0];
    if (c->fake_timeouts > 0 && timeouts && !c->async_pending) {  // debug: IE_FAKE_TIMEOUTS
        c->fake_timeouts--;
        c->fake_fired = true;
        t++;
    }
    if (timeouts) *timeouts = t;
    if (fallbacks) *fallbacks = f;
    std::memcpy(c->err_seen, e, sizeof(e));
    const unsigned pending = c->async_pending;
    const char* what = c->async_what;
    c->async_pending = 0;
    c->async_what = nullptr;
    if (t && pending) {
        // a launch that returned without a read-back timed out: its output is invalid and there is
        // nothing to re-run here -- fail loudly (later launches order their tiles by ticket)
        c->use_ticket = true;
        return fail(c, IE_EDEVICE, std::string(kTimedOut) + " in an earlier asynchronous " + (what ? what : "launch") +
                                       " (" + std::to_string(pending) + " unchecked launch(es)); its output is invalid");
    }
    return IE_OK;
}

// An asynchronous launch returned without reading the error counters: the next read (ie_sync or
// any synchronous call) checks it.
void note_async(ie_ctx* c, const char* what) {
    c->async_pending++;
    c->async_what = what;
}

int check_dims(ie_ctx* c, int w, int h, int nframes) {
    if (!c->n) return fail(c, IE_ENOQUANT, "ie_set_quant has not been called");
    if (w <= 0 || h <= 0 || w % c->n || h % c->n)
        return fail(c, IE_EINVAL, "width/height must be positive multiples of the block size");
    if (w > 32767 || h > 32767) return fail(c, IE_EINVAL, "width/height exceed the 15-bit header fields");
    if (nframes <= 0) return fail(c, IE_EINVAL, "nframes must be > 0");
    return IE_OK;
}

int check_frames(ie_ctx* c, int w, int h, int nframes, size_t stride, size_t frame_pitch) {
    int r = check_dims(c, w, h, nframes);
    if (r) return r;
    if (stride < size_t(w)) return fail(c, IE_EINVAL, "stride < width");
    if (nframes > 1 && frame_pitch < frames_span(1, 0, stride, w, h))
        return fail(c, IE_EINVAL, "frame_pitch smaller than a frame");
    return IE_OK;
}

int stage_in(ie_ctx* c, const uint8_t* src, bool src_dev, size_t bytes, const uint8_t** dsrc) {
    *dsrc = src;
    if (src_dev || !bytes) return IE_OK;
    int r = c->d_in.reserve(c, bytes);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(c->d_in, src, bytes, hipMemcpyHostToDevice, c->stream));
    *dsrc = c->d_in;
    return IE_OK;
}

}  // namespace iec

extern "C" {

int ie_create(int device, ie_ctx** out) {
    if (!out) return IE_EINVAL;
    *out = nullptr;
    ie_ctx* c = new ie_ctx();
    c->device = device;
    int r = IE_OK;
    auto chk = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && r == IE_OK) r = fail(c, IE_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    };
    chk(hipSetDevice(device), "hipSetDevice");
    // A BLOCKING stream: it orders with the legacy default (NULL) stream, so device buffers a caller
    // (e.g. PyTorch's default stream) filled just before a call are complete when the call's kernels
    // read them, and vice versa.  (Callers with their own streams use ie_set_stream.)
    if (r == IE_OK) r = c->own.create(c, hipStreamDefault);
    c->stream = c->own;
    // Debug switch: order tiles by the atomic ticket from the first launch (exercises the
    // timeout-recovery path, which dispatch order otherwise never needs)
    if (const char* ft = getenv("IE_FORCE_TICKET")) c->use_ticket = atoi(ft) != 0;
    // Debug switch: the next k synchronous error checks report a look-back timeout (exercises the
    // redo-in-ticket-mode paths and their output clearing)
    if (const char* ft = getenv("IE_FAKE_TIMEOUTS")) c->fake_timeouts = atoi(ft);
    if (r == IE_OK) r = c->d_tab.reserve(c, 1);
    if (r == IE_OK) r = c->h_tab.reserve(c, 1);
    if (r == IE_OK) r = c->d_ticket.reserve(c, 1);
    if (r == IE_OK) chk(hipMemset(c->d_ticket, 0, sizeof(unsigned long long)), "hipMemset(ticket)");
    if (r == IE_OK) r = c->d_err.reserve(c, kErrWords);
    if (r == IE_OK) chk(hipMemset(c->d_err, 0, kErrWords * sizeof(unsigned)), "hipMemset(err)");
    if (r == IE_OK) r = c->d_code.reserve(c, 2 * 256);
    if (r == IE_OK) r = c->h_code.reserve(c, 2 * 256);
    if (r == IE_OK) r = c->d_hist.reserve(c, 256);
    if (r == IE_OK) r = c->d_misc.reserve(c, 8);
    if (r == IE_OK) r = c->d_first.reserve(c, 256);
    if (r != IE_OK) {
        std::fprintf(stderr, "ie_create: %s\n", c->err.c_str());
        ie_destroy(c);
        return r;
    }
    *out = c;
    return IE_OK;
}

int ie_destroy(ie_ctx* c) {
    if (!c) return IE_OK;
    (void)hipSetDevice(c->device);
    if (c->own) (void)hipStreamSynchronize(c->own);
    if (c->stream && c->stream != c->own) (void)hipStreamSynchronize(c->stream);
    if (c->tab_stream) (void)hipStreamSynchronize(c->tab_stream);
    pipe_free(c->pipe);
    delete c;  // the buffers and events, then the streams
    return IE_OK;
}

const char* ie_last_error(const ie_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ie_set_error(ie_ctx* c, const char* msg) {
    if (!c) return IE_EINVAL;
    c->err = msg ? msg : "";
    return IE_OK;
}

int ie_set_stream(ie_ctx* c, void* s) {
    if (!c) return IE_EINVAL;
    c->stream = s ? static_cast<hipStream_t>(s) : c->own.s;
    return IE_OK;
}

int ie_sync(ie_ctx* c) {
    if (!c) return IE_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned timeouts = 0;
    int r = read_errors(c, &timeouts, nullptr);  // fails if an unchecked launch timed out
    if (r) return r;
    if (timeouts) {  // (no asynchronous launch pending: a synchronous caller already re-ran it)
        c->use_ticket = true;
        return lookback_failed(c);
    }
    return IE_OK;
}

int ie_set_quant(ie_ctx* c, const uint16_t* q, int n) {
    if (!c || !q) return IE_EINVAL;
    if (n != 4 && n != 8) return fail(c, IE_EINVAL, "block size must be 4 or 8");
    for (int k = 0; k < n * n; k++)
        if (q[k] == 0) return fail(c, IE_EINVAL, "quantisation matrix entries must be > 0");
    if (c->n == n && std::memcmp(c->q, q, sizeof(uint16_t) * n * n) == 0) return IE_OK;  // unchanged
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // tables may be in use by a running launch
    if (!build_tables(n, q, c->h_tab)) return fail(c, IE_EINVAL, "FP32 transform does not match the reference map");
    HIPCHK(c, hipMemcpy(c->d_tab, c->h_tab, sizeof(ie::EncTables), hipMemcpyHostToDevice));
    c->n = n;
    std::memcpy(c->q, q, sizeof(uint16_t) * n * n);
    return IE_OK;
}

int ie_set_stage_timing(ie_ctx* c, int on) {
    if (!c) return IE_EINVAL;
    c->stage_timing = on != 0;
    if (!c->stage_timing) c->stage_rec[0] = c->stage_rec[1] = false;  // (stale marks are not reported)
    return IE_OK;
}

int ie_last_stage_ms(ie_ctx* c, int stage, float* ms) {
    if (!c || !ms || stage < 0 || stage > 1) return IE_EINVAL;
    if (!c->stage_rec[stage]) return fail(c, IE_EINVAL, "no batched Huffman stage recorded yet");
    HIPCHK(c, hipEventSynchronize(c->stage_ev[2 * stage + 1]));
    HIPCHK(c, hipEventElapsedTime(ms, c->stage_ev[2 * stage], c->stage_ev[2 * stage + 1]));
    return IE_OK;
}

int ie_cos_table(ie_ctx* c, double* out) {
    if (!c || !out) return IE_EINVAL;
    if (c->n == 0) return fail(c, IE_ENOQUANT, "ie_set_quant not called");
    // read back from the DEVICE table: the values every kernel's FP64 path multiplies with
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, reinterpret_cast<const char*>(c->d_tab.get()) + offsetof(ie::EncTables, c),
                        sizeof(double) * size_t(c->n) * size_t(c->n), hipMemcpyDeviceToHost));
    return IE_OK;
}

int ie_is_device_ptr(const void* p) { return is_device_ptr(p) ? 1 : 0; }

int ie_malloc(ie_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return IE_EINVAL;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(out, bytes ? bytes : 4));
    return IE_OK;
}

int ie_free(ie_ctx* c, void* p) {
    if (!c) return IE_EINVAL;
    if (!p) return IE_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(p));
    return IE_OK;
}

int ie_memcpy(ie_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return IE_EINVAL;
    if (!bytes) return IE_OK;
    const bool dd = is_device_ptr(dst), sd = is_device_ptr(src);
    const hipMemcpyKind k = dd ? (sd ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                               : (sd ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
    if (k == hipMemcpyHostToHost) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memcpy(dst, src, bytes);
        return IE_OK;
    }
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, k, c->stream));
    if (k != hipMemcpyDeviceToDevice) HIPCHK(c, hipStreamSynchronize(c->stream));
    return IE_OK;
}

int ie_memset(ie_ctx* c, void* dst, int value, size_t bytes) {
    if (!c || (bytes && !dst)) return IE_EINVAL;
    if (!bytes) return IE_OK;
    if (!is_device_ptr(dst)) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memset(dst, value, bytes);
        return IE_OK;
    }
    HIPCHK(c, hipMemsetAsync(dst, value, bytes, c->stream));
    return IE_OK;
}

int ie_host_alloc(ie_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return IE_EINVAL;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc(out, bytes ? bytes : 4));
    return IE_OK;
}

int ie_host_free(ie_ctx* c, void* p) {
    if (!c) return IE_EINVAL;
    if (!p) return IE_OK;
    HIPCHK(c, hipHostFree(p));
    return IE_OK;
}

}  // extern "C"
