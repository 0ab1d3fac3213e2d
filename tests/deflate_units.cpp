// deflate_units.cpp — unikmer_amd/csrc/ukm_huff.h (the code construction, the block header and the CRC arithmetic that
// ukm_deflate's kernels share with the host) as a stand-alone program under the sanitizers: for every input the lengths are
// built and held to their contract, one chunk is assembled serially with the shared header writer, and zlib's raw inflate
// must give the input back; then unik::OutStream's device-gzip mode (unikmer_amd/host/unik.hpp) is fed such chunks between
// small writes, in several orders, and unik::InStream must read the whole back.  Needs neither the library nor a device.
// argv[1]: a directory for those files; a file body.bin there is one more input (its first DFL_CHUNK bytes).  Prints OK.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ukm_huff.h"
#include "unik.hpp"

#ifndef DFL_CHUNK
#error "compile with -DDFL_CHUNK=<the kernels' chunk size>"
#endif

namespace H = ukm_huff;
typedef std::vector<uint8_t> Bytes;

#define CHECK(cond, ...)                              \
    do {                                              \
        if (!(cond)) {                                \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);             \
            fprintf(stderr, "\n");                    \
            exit(1);                                  \
        }                                             \
    } while (0)

// limit, Kraft sum exactly 1, every symbol that occurs has a length; returns the longest length
static int check_contract(const char *what, const uint32_t *freq, const uint8_t *len, int n, int limit) {
    uint64_t kraft = 0;
    int longest = 0, used = 0;
    for (int s = 0; s < n; s++) {
        CHECK(len[s] <= limit, "%s: symbol %d has length %d > %d", what, s, len[s], limit);
        if (freq[s]) {
            used++;
            CHECK(len[s] > 0, "%s: symbol %d occurs %u times and has no code", what, s, freq[s]);
        }
        if (len[s]) kraft += 1ull << (limit - len[s]);
        if (len[s] > longest) longest = len[s];
    }
    CHECK(kraft == 1ull << limit, "%s: Kraft sum %llu / %llu", what, (unsigned long long)kraft, 1ull << limit);
    if (used >= 2)
        for (int s = 0; s < n; s++) CHECK(freq[s] || !len[s], "%s: symbol %d never occurs and has a code", what, s);
    return longest;
}

static Bytes inflate_raw(const Bytes &in, size_t expect) {
    Bytes out(expect + 64);
    z_stream z;
    memset(&z, 0, sizeof z);
    CHECK(inflateInit2(&z, -15) == Z_OK, "inflateInit2");
    z.next_in = const_cast<Bytef *>(in.data());
    z.avail_in = (uInt)in.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    const int rc = inflate(&z, Z_FINISH);
    CHECK(rc == Z_STREAM_END, "inflate: %d (%s)", rc, z.msg ? z.msg : "");
    CHECK(z.avail_in == 0, "inflate left %u bytes", z.avail_in);
    out.resize(z.total_out);
    inflateEnd(&z);
    return out;
}

// one chunk as the write kernel lays it out, serially; *header_bytes: what the block header took
static Bytes encode_chunk(const char *what, const Bytes &src, int *longest, double *header_bytes) {
    static H::HeaderScratch hs;
    uint32_t freq[H::LIT_SYMS] = {0};
    uint8_t len[H::LIT_SYMS];
    uint16_t code[H::LIT_SYMS];
    for (uint8_t b : src) freq[b]++;
    freq[H::EOB] = 1;
    H::build_lengths(freq, H::LIT_SYMS, H::LIT_LIMIT, &hs.lengths, len);
    *longest = check_contract(what, freq, len, H::LIT_SYMS, H::LIT_LIMIT);
    H::assign_codes(len, H::LIT_SYMS, code);
    H::BitWriter count = {nullptr, 0};
    H::block_header(len, &hs, &count);
    check_contract(what, hs.cl_freq, hs.cl_len, H::CL_SYMS, H::CL_LIMIT);
    uint64_t literal_bits = 0;
    for (int s = 0; s < 256; s++) literal_bits += (uint64_t)freq[s] * len[s];
    Bytes out(H::dynamic_bytes(count.pos, literal_bits, len[H::EOB]), 0);
    H::BitWriter w = {out.data(), 0};
    H::block_header(len, &hs, &w);
    CHECK(w.pos == count.pos, "%s: the header counts %llu bits and writes %llu", what, (unsigned long long)count.pos, (unsigned long long)w.pos);
    *header_bytes = (double)count.pos / 8;
    for (uint8_t b : src) w.put(code[b], len[b]);
    w.put(code[H::EOB], len[H::EOB]);
    w.put(0, 3);  // the empty stored block
    w.pos = (w.pos + 7) & ~7ull;
    w.put(0xFFFF0000u, 32);
    CHECK(w.pos == 8 * (uint64_t)out.size(), "%s: %llu bits in %zu bytes", what, (unsigned long long)w.pos, out.size());
    return out;
}

static void round_trip(const char *what, const Bytes &src, int want_longest = 0) {
    int longest = 0;
    double hb = 0;
    Bytes z = encode_chunk(what, src, &longest, &hb);
    if (want_longest) CHECK(longest == want_longest, "%s: longest code %d, expected %d", what, longest, want_longest);
    z.push_back(3);  // the final empty block
    z.push_back(0);
    const Bytes back = inflate_raw(z, src.size());
    CHECK(back == src, "%s: inflate gives %zu bytes, not the input's %zu", what, back.size(), src.size());
    fprintf(stderr, "%-22s %6zu -> %6zu bytes, header %.1f, longest code %d\n", what, src.size(), z.size() - 2, hb, longest);
}

static uint32_t raw_crc(const uint8_t *p, size_t n) {
    uint32_t c = 0;
    for (size_t i = 0; i < n; i++) c = H::crc_table_entry((c ^ p[i]) & 255u) ^ (c >> 8);
    return c;
}

int main(int argc, char **argv) {
    static_assert(DFL_CHUNK <= 65535, "a chunk must fit one stored block");
    round_trip("one byte", Bytes(1, 0x41));
    round_trip("one value", Bytes(DFL_CHUNK, 7), 1);
    round_trip("one value, zero", Bytes(DFL_CHUNK, 0), 1);
    {
        Bytes b(1000, 1);
        for (size_t i = 0; i < b.size(); i += 3) b[i] = 200;
        round_trip("two values", b);
    }
    {
        Bytes b(256);
        for (int i = 0; i < 256; i++) b[i] = (uint8_t)i;
        round_trip("all values once", b);
    }
    // Fibonacci frequencies 1, 1, 2, 3 ... 10946 over 21 byte values: 28656 bytes.  End-of-block is a third symbol of weight
    // 1, so every merge meets a tie and a Huffman tree that resolves ties towards the leaf is two interleaved chains, 11
    // deep: the limit does not act here.  It does on the next input.
    const uint32_t fib_count = 21;
    std::vector<uint32_t> fib(fib_count);
    {
        Bytes b;
        for (uint32_t i = 0; i < fib_count; i++) {
            fib[i] = i < 2 ? 1 : fib[i - 1] + fib[i - 2];
            b.insert(b.end(), fib[i], (uint8_t)(37 + 5 * i));
        }
        CHECK(b.size() == 28656 && fib.back() == 10946, "the Fibonacci input is %zu bytes", b.size());
        static_assert(DFL_CHUNK >= 28656, "the Fibonacci input must fit one chunk");
        round_trip("Fibonacci", b);
        // 1, 2, 3, 5 ... 2584 over 17 byte values: with end-of-block the weights are the Fibonacci numbers themselves, no
        // merge meets a tie, the unlimited tree is one chain 17 deep, and the limit of 15 must act
        Bytes c;
        for (uint32_t i = 0; i < 17; i++) c.insert(c.end(), fib[i + 1], (uint8_t)(250 - 9 * i));
        CHECK(c.size() == 6763, "the chain input is %zu bytes", c.size());
        round_trip("Fibonacci chain", c, H::LIT_LIMIT);
    }
    {   // the same run of lengths on the 19-symbol alphabet with limit 7
        static H::Scratch S;
        uint32_t freq[H::CL_SYMS];
        uint8_t len[H::CL_SYMS];
        for (int i = 0; i < H::CL_SYMS; i++) freq[i] = fib[(size_t)i];
        H::build_lengths(freq, H::CL_SYMS, H::CL_LIMIT, &S, len);
        CHECK(check_contract("Fibonacci, limit 7", freq, len, H::CL_SYMS, H::CL_LIMIT) == H::CL_LIMIT, "the limit of 7 did not act");
        for (int i = 1; i < H::CL_SYMS; i++) CHECK(len[i] <= len[i - 1], "a more frequent symbol has a longer code");
        freq[3] = 0;  // ... and with a symbol that does not occur
        H::build_lengths(freq, H::CL_SYMS, H::CL_LIMIT, &S, len);
        check_contract("Fibonacci, limit 7, 18 symbols", freq, len, H::CL_SYMS, H::CL_LIMIT);
        CHECK(len[3] == 0, "a symbol that never occurs has a code");
    }
    if (argc > 1) {
        const std::string path = std::string(argv[1]) + "/body.bin";
        if (FILE *f = fopen(path.c_str(), "rb")) {
            Bytes b(DFL_CHUNK);
            b.resize(fread(b.data(), 1, b.size(), f));
            fclose(f);
            CHECK(!b.empty(), "%s is empty", path.c_str());
            round_trip("sorted body", b);
        }
    }
    {   // the CRC arithmetic against zlib
        Bytes a(1000), b(77777);
        for (size_t i = 0; i < a.size(); i++) a[i] = (uint8_t)(i * 31 + 7);
        for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)((i * i) >> 3);
        const uint32_t ca = (uint32_t)crc32(0, a.data(), (uInt)a.size()), cb = (uint32_t)crc32(0, b.data(), (uInt)b.size());
        const uint32_t cab = (uint32_t)crc32(ca, b.data(), (uInt)b.size());
        CHECK(H::crc_combine(ca, cb, b.size()) == cab, "crc_combine");
        CHECK(H::crc_append_raw(ca, raw_crc(b.data(), b.size()), b.size()) == cab, "crc_append_raw");
        CHECK(H::crc_append_raw(0, raw_crc(b.data(), b.size()), b.size()) == cb, "crc_append_raw from nothing");
        // a raw CRC is the XOR of its slices' raw CRCs, each times x^(8 * bytes behind it)
        uint32_t x = 0;
        for (size_t at = 0; at < b.size(); at += 128) {
            const size_t l = b.size() - at < 128 ? b.size() - at : 128;
            x ^= H::crc_mul(raw_crc(b.data() + at, l), H::crc_x8n(b.size() - at - l));
        }
        CHECK(x == raw_crc(b.data(), b.size()), "slices");
        CHECK(H::crc_combine(ca, 0, 0) == ca, "combine with nothing");
    }
    if (argc > 1) {   // OutStream in device-gzip mode: small writes through zlib, deflated chunks as they are, any order of calls
        Bytes head(92, 0x5a), tail(13, 0x11), body;
        for (int i = 0; i < 50000; i++) body.push_back((uint8_t)((i % 7) * (i % 5)));
        int longest;
        double hb;
        const Bytes frag = encode_chunk("stream", Bytes(body.begin(), body.begin() + DFL_CHUNK), &longest, &hb);
        const Bytes frag2 = encode_chunk("stream", Bytes(body.begin() + DFL_CHUNK, body.end()), &longest, &hb);
        const uint32_t c1 = (uint32_t)crc32(0, body.data(), DFL_CHUNK), c2 = (uint32_t)crc32(0, body.data() + DFL_CHUNK, (uInt)(body.size() - DFL_CHUNK));
        for (int order = 0; order < 4; order++) {
            const std::string path = std::string(argv[1]) + "/stream" + std::to_string(order) + ".gz";
            Bytes want;
            {
                unik::OutStream os(path, true, order == 3 ? 9 : -1, true);
                CHECK(os.device_gzip(), "device-gzip mode was asked for");
                auto small = [&](const Bytes &b) { os.write(b.data(), b.size()); want.insert(want.end(), b.begin(), b.end()); };
                auto big = [&]() {
                    os.write_deflated(frag.data(), frag.size(), c1, DFL_CHUNK);
                    os.write_deflated(frag2.data(), frag2.size(), c2, body.size() - DFL_CHUNK);
                    want.insert(want.end(), body.begin(), body.end());
                };
                if (order == 0) { small(head); big(); small(tail); }
                if (order == 1) { big(); small(tail); }
                if (order == 2) { small(head); small(tail); big(); big(); }
                if (order == 3) { small(head); big(); }
                os.close();
            }
            unik::InStream in(path);
            Bytes got(want.size() + 10);
            got.resize(in.read(got.data(), got.size()));
            CHECK(in.gzipped(), "%s is not gzip", path.c_str());
            CHECK(got == want, "order %d: %zu bytes read back, %zu written", order, got.size(), want.size());
        }
        unik::OutStream off(std::string(argv[1]) + "/level0.gz", true, 0, true);  // level 0 stays on zlib's own writer
        CHECK(!off.device_gzip(), "--compression-level 0 must not take the device path");
    }
    printf("OK\n");
    return 0;
}
