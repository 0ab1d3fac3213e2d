// The host codec of unikmer_amd/host/unik.hpp alone, timed: Reader::read_all of a file, then the Writer's record loop to a
// second file (uncompressed).  tools/bench_codec.py builds and runs it beside the device codec.
//   codec_host_timer <in.unik> <out.unik>   ->   one JSON line: records, read_ms, write_ms
#include <chrono>
#include <cstdio>

#include "unik.hpp"

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::vector<uint64_t> codes;
    std::vector<uint32_t> taxids;
    unik::Header h;
    const double t0 = now_ms();
    {
        unik::Reader r(argv[1]);
        h = r.h;
        r.read_all(codes, h.is_include_taxid() ? &taxids : nullptr);
    }
    const double t1 = now_ms();
    {
        unik::OutStream os(argv[2], false, -1);
        unik::Writer w(os, h.k, h.flag);
        w.h = h;
        for (size_t i = 0; i < codes.size(); i++) {
            if (h.is_include_taxid()) w.write_code_with_taxid(codes[i], taxids[i]);
            else w.write_code(codes[i]);
        }
        w.flush();
        os.close();
    }
    const double t2 = now_ms();
    printf("{\"records\": %zu, \"read_ms\": %.1f, \"write_ms\": %.1f}\n", codes.size(), t1 - t0, t2 - t1);
    return 0;
}
