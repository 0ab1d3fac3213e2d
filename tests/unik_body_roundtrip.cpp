// Stand-alone check of unik::Reader::read_body / unik::Writer::write_body (unikmer_amd/host/unik.hpp), built by
// tests/test_unik_codec_cpu.py with -fsanitize=address,undefined: a file written record by record is read once by the
// record loop and once in bulk; the bulk body written behind the same header gives the same file, which reads back as
// the same records.  usage: unik_body_roundtrip <scratch directory>
#include <cstdio>
#include <fstream>
#include <iterator>

#include "unik.hpp"

static std::vector<uint8_t> slurp(const std::string &p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int round_trip(const std::string &dir, uint32_t mode, int k, uint64_t n, bool compress) {
    const std::string a = dir + "/a.unik", b = dir + "/b.unik";
    std::vector<uint64_t> codes;
    std::vector<uint32_t> taxids;
    uint64_t c = 0x0123456789ABCDEFull, x = 88172645463325252ull;  // (the first delta takes 8 bytes)
    for (uint64_t i = 0; i < n; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        c += x >> (16 + (i % 6) * 8);  // deltas of 1..6 bytes; the sum stays below 2^64
        codes.push_back(k < 32 && (mode & unik::UnikCompact) ? c & ((1ull << (2 * k)) - 1) : c);
        taxids.push_back((uint32_t)(x >> 40));
    }
    {
        unik::OutStream os(a, compress, -1);
        unik::Writer w(os, k, mode);
        w.set_max_taxid(0xFFFFFF);
        w.set_number(n);
        for (uint64_t i = 0; i < n; i++) w.write_code_with_taxid(codes[i], taxids[i]);
        w.flush();
        os.close();
    }
    std::vector<uint64_t> c1, c2;
    std::vector<uint32_t> t1, t2;
    unik::Header h;
    {
        unik::Reader r(a);
        h = r.h;
        r.read_all(c1, &t1);
    }
    std::vector<uint8_t> body;
    {
        unik::Reader r(a);
        r.read_body(body);
    }
    {
        unik::OutStream os(b, compress, -1);
        unik::Writer w(os, k, mode);
        w.h = h;
        w.write_body(body.data(), body.size());
        w.flush();
        os.close();
    }
    {
        unik::Reader r(b);
        r.read_all(c2, &t2);
    }
    const bool tx = (mode & unik::UnikIncludeTaxID) != 0;
    if (c1 != codes || c2 != codes) { fprintf(stderr, "codes differ (mode %u)\n", mode); return 1; }
    if (tx && (t1.size() != n || t2 != t1)) { fprintf(stderr, "taxids differ (mode %u)\n", mode); return 1; }
    for (uint64_t i = 0; tx && i < n; i++)
        if (t1[i] != (taxids[i] & 0xFFFFFF)) { fprintf(stderr, "taxid %llu differs\n", (unsigned long long)i); return 1; }
    if (!compress && slurp(a) != slurp(b)) { fprintf(stderr, "files differ (mode %u)\n", mode); return 1; }
    if (!compress && slurp(a).size() != 100 + body.size()) { fprintf(stderr, "body size (mode %u)\n", mode); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const std::string dir = argv[1];
    int bad = 0;
    for (int compress = 0; compress < 2; compress++) {
        bad |= round_trip(dir, unik::UnikSorted | unik::UnikIncludeTaxID, 31, 100001, compress);
        bad |= round_trip(dir, unik::UnikSorted, 31, 4096, compress);
        bad |= round_trip(dir, unik::UnikIncludeTaxID, 21, 777, compress);
        bad |= round_trip(dir, unik::UnikCompact, 11, 1000, compress);
        bad |= round_trip(dir, unik::UnikSorted, 31, 0, compress);
    }
    if (bad) return 1;
    puts("OK");
    return 0;
}
