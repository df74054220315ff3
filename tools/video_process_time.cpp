// tools/video_process_time.cpp -- wall time of dc::VideoEncoder::process (Huffman off) on a
// .raw/YUV420 video file, the way the encoder command line runs it.  Built and driven by
// tools/video_stream_ab.py against the libie_host.so of two builds in turn.
//
//   video_process_time <in.yuv> <w> <h> <matrix.txt> <gop> <merange> <warmup> <reps>
//
// Every repetition constructs a VideoEncoder and times process() with a host clock (process ends
// with the finished file in host memory, after the stream's last synchronisation).  Prints one
// line per timed repetition: "ms <time> bytes <size> fnv <hash of the result>".
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "ie_host.hpp"

int main(int argc, char** argv) {
    if (argc < 9) return 1;
    dc::MatrixReader<4> m;
    if (!m.read(argv[4])) return 4;
    dc::EncodeOptions opt;
    opt.huffman = false;
    const int warmup = std::atoi(argv[7]), reps = std::atoi(argv[8]);
    for (int i = 0; i < warmup + reps; i++) {
        dc::VideoEncoder enc(argv[1], "unused.enc", uint16_t(std::atoi(argv[2])), uint16_t(std::atoi(argv[3])), true, m,
                             uint16_t(std::atoi(argv[5])), uint16_t(std::atoi(argv[6])), opt);
        const auto t0 = std::chrono::steady_clock::now();
        if (!enc.process()) {
            std::fprintf(stderr, "%s\n", enc.error().c_str());
            return 7;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        uint64_t hash = 1469598103934665603ull;
        for (uint8_t b : enc.result()) hash = (hash ^ b) * 1099511628211ull;
        if (i >= warmup) std::printf("ms %.3f bytes %zu fnv %016llx\n", ms, enc.result().size(), (unsigned long long)hash);
    }
    return 0;
}
