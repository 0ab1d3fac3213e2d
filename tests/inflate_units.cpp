// inflate_units.cpp — the host pieces of the driver's device gunzip path (unikmer_amd/host/unik.hpp: unik::GzInput) as a
// stand-alone program under the sanitizers: gzip framing, the Z_BLOCK search for the body's start on OutStream device-gzip
// files written in four call orders, the dictionary resume, the trailer check, and the refusals.  The device is stood in for
// by fake_inflate: the block parser the kernels use (unikmer_amd/csrc/ukm_inflate.h, compiled for the host) run the way
// ukm_inflate.hip runs it -- candidates, a walk per candidate, the chain, checkpoints, a decode per checkpoint -- and that
// stand-in is itself held to zlib first.  Needs neither the library nor a device.  argv[1]: a directory for the files.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ukm_inflate.h"
#include "unik.hpp"

namespace P = ukm_puff;
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

// ukm_inflate's contract, serially, in the kernels' steps.  src is copied to the end of an exact allocation, `misalign` bytes
// behind its aligned start: a load behind src[0, n) is the address sanitizer's to report.
static void fake_inflate(const uint8_t *src_in, uint64_t n, Bytes *out, uint64_t *consumed, int misalign = 0) {
    out->clear();
    *consumed = 0;
    if (n == 0) return;
    uint8_t *slab = (uint8_t *)malloc((size_t)n + (size_t)misalign);
    const uint8_t *src = (const uint8_t *)memcpy(slab + misalign, src_in, (size_t)n);
    std::vector<uint64_t> cand(1, 0);
    for (uint64_t p = 0; p + 4 <= n; p++)
        if (src[p] == 0 && src[p + 1] == 0 && src[p + 2] == 0xFF && src[p + 3] == 0xFF) cand.push_back(p + 4);
    static P::Table table;
    static uint8_t lens[P::LENS];
    static uint16_t lut[P::LUT_SIZE];  // the walks decode through the lookup table, the checkpoints below bit by bit
    std::vector<P::SegResult> seg;
    for (uint64_t c : cand) seg.push_back(P::walk_segment(src, n, c, ~0ull, &table, lens, lut, [](uint64_t, uint64_t, uint64_t, uint32_t) {}));
    std::vector<P::Checkpoint> cps;
    uint64_t total = 0;
    for (size_t i = 0;;) {
        const P::SegResult &r = seg[i];
        if (r.end <= cand[i]) break;
        const size_t before = cps.size();
        const P::SegResult again = P::walk_segment(src, n, cand[i], r.end, &table, lens, i % 2 ? lut : nullptr, [&](uint64_t bit, uint64_t hdr, uint64_t o, uint32_t len) {
            P::Checkpoint c = {bit, hdr, total + o, len, 0};
            cps.push_back(c);
        });
        CHECK(!again.early && again.end == r.end && again.out == r.out, "the second walk of the segment at %llu differs", (unsigned long long)cand[i]);
        CHECK(cps.size() - before == r.ncp, "segment at %llu: %zu checkpoints, %llu counted", (unsigned long long)cand[i], cps.size() - before,
              (unsigned long long)r.ncp);
        total += r.out;
        *consumed = r.end;
        if (r.early) break;
        const auto it = std::lower_bound(cand.begin() + (std::ptrdiff_t)i + 1, cand.end(), r.end);
        if (it == cand.end() || *it != r.end) break;
        i = (size_t)(it - cand.begin());
    }
    out->assign((size_t)total, 0xEE);
    uint64_t at = 0;
    for (const P::Checkpoint &c : cps) {  // each on its own, as a lane of the write kernel
        CHECK(c.out == at && c.n >= 1 && c.n <= P::CP_BYTES, "checkpoints are consecutive output");
        at += c.n;
        if (c.hdr == P::STORED_CP) {
            memcpy(out->data() + c.out, src + (c.bit >> 3), c.n);
            continue;
        }
        P::BitReader br;
        br.src = src;
        br.n_bytes = n;
        br.seek(c.hdr);
        uint32_t h = 0;
        CHECK(br.take(3, &h) && (h == 2 || h == 4), "a checkpoint's header");
        CHECK(P::build_table(&br, (int)(h >> 1), &table, lens), "a checkpoint's table");
        br.seek(c.bit);
        for (uint32_t i = 0; i < c.n; i++) {
            const int s = P::decode_symbol(&br, &table);
            CHECK(s >= 0 && s < 256, "a checkpoint's symbol");
            (*out)[c.out + i] = (uint8_t)s;
        }
    }
    CHECK(at == total, "the checkpoints cover the output");
    free(slab);
}

static Bytes deflate_raw(const Bytes &in, int level, int mem_level, int strategy, size_t chunk, int flush, bool finish, const Bytes *dict = nullptr) {
    z_stream z;
    memset(&z, 0, sizeof z);
    CHECK(deflateInit2(&z, level, Z_DEFLATED, -15, mem_level, strategy) == Z_OK, "deflateInit2");
    if (dict) CHECK(deflateSetDictionary(&z, dict->data(), (uInt)dict->size()) == Z_OK, "deflateSetDictionary");
    Bytes out(deflateBound(&z, (uLong)in.size()) + 64 + 16 * (in.size() / (chunk ? chunk : 1) + 1));
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    for (size_t at = 0; at < in.size() || at == 0; at += chunk) {
        const size_t l = std::min(chunk, in.size() - at);
        z.next_in = const_cast<Bytef *>(in.data()) + at;
        z.avail_in = (uInt)l;
        CHECK(deflate(&z, flush) == Z_OK && z.avail_in == 0, "deflate");
        if (in.empty()) break;
    }
    if (finish) CHECK(deflate(&z, Z_FINISH) == Z_STREAM_END, "deflate finish");
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

static Bytes inflate_with_dict(const uint8_t *in, size_t n, const Bytes &dict, size_t room) {
    z_stream z;
    memset(&z, 0, sizeof z);
    CHECK(inflateInit2(&z, -15) == Z_OK, "inflateInit2");
    if (!dict.empty()) CHECK(inflateSetDictionary(&z, dict.data(), (uInt)dict.size()) == Z_OK, "inflateSetDictionary");
    Bytes out(room + 64);
    z.next_in = const_cast<Bytef *>(in);
    z.avail_in = (uInt)n;
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    const int rc = inflate(&z, Z_FINISH);
    CHECK(rc == Z_STREAM_END && z.avail_in == 0, "inflate with dictionary: %d (%s)", rc, z.msg ? z.msg : "");
    out.resize(z.total_out);
    inflateEnd(&z);
    return out;
}

static uint32_t g_rng = 12345;
static uint32_t rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

static void parser_against_zlib() {
    const size_t CH = 32768;
    std::vector<std::pair<const char *, Bytes>> inputs;
    {
        Bytes b(2 * CH + 777);
        for (auto &v : b) {  // skewed: the minimum of three draws
            v = (uint8_t)std::min(std::min(rnd() & 255u, rnd() & 255u), rnd() & 255u);
        }
        for (size_t i = 5000; i < 6000; i++) b[i] = (uint8_t)rnd();  // (memLevel 1 stores this stretch, unaligned)
        inputs.push_back({"skewed", b});
        Bytes r(2 * CH + 5);
        for (auto &v : r) v = (uint8_t)rnd();
        inputs.push_back({"random", r});
        inputs.push_back({"three", Bytes{'a', 'b', 'c'}});
        inputs.push_back({"one value", Bytes(3 * CH + 1, 7)});
        Bytes d;  // delta-like: small values with rare large ones
        for (size_t i = 0; i < 3 * CH + 11; i++) d.push_back((uint8_t)(rnd() % 16 == 0 ? rnd() : rnd() % 5));
        inputs.push_back({"deltas", d});
    }
    for (auto &in : inputs) {
        for (int mem_level : {9, 8, 1}) {
            const Bytes z = deflate_raw(in.second, 6, mem_level, Z_HUFFMAN_ONLY, CH, Z_FULL_FLUSH, false);
            for (int misalign : {0, 1, 3}) {
                Bytes out;
                uint64_t consumed = 0;
                fake_inflate(z.data(), z.size(), &out, &consumed, misalign);
                CHECK(consumed == z.size(), "%s, memLevel %d: consumed %llu of %zu", in.first, mem_level, (unsigned long long)consumed, z.size());
                CHECK(out == in.second, "%s, memLevel %d: the output differs", in.first, mem_level);
            }
            // cut anywhere: the prefix is what zlib gives for the consumed bytes, and nothing outside src is read
            for (int t = 0; t < 24; t++) {
                const size_t cut = t < 12 && z.size() > (size_t)t + 1 ? z.size() - 1 - (size_t)t : rnd() % z.size();
                Bytes out;
                uint64_t consumed = 0;
                fake_inflate(z.data(), cut, &out, &consumed);
                CHECK(consumed <= cut && out.size() <= in.second.size() && std::equal(out.begin(), out.end(), in.second.begin()),
                      "%s, memLevel %d, cut at %zu: not a prefix", in.first, mem_level, cut);
                Bytes fin(z.begin(), z.begin() + (std::ptrdiff_t)consumed);
                fin.push_back(3);
                fin.push_back(0);
                CHECK(inflate_with_dict(fin.data(), fin.size(), Bytes(), in.second.size()) == out, "%s, memLevel %d, cut at %zu: zlib disagrees", in.first,
                      mem_level, cut);
            }
            // one flipped bit anywhere: the run ends, inside the source, with a prefix zlib agrees on
            for (int t = 0; t < 25; t++) {
                Bytes bad = z;
                bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8));
                Bytes out;
                uint64_t consumed = 0;
                fake_inflate(bad.data(), bad.size(), &out, &consumed);
                Bytes fin(bad.begin(), bad.begin() + (std::ptrdiff_t)consumed);
                fin.push_back(3);
                fin.push_back(0);
                CHECK(inflate_with_dict(fin.data(), fin.size(), Bytes(), out.size() + 16) == out, "%s, memLevel %d: a flipped bit, zlib disagrees", in.first,
                      mem_level);
            }
        }
        // a stream with matches: nothing is taken
        const Bytes z6 = deflate_raw(in.second, 6, 8, Z_DEFAULT_STRATEGY, in.second.size(), Z_NO_FLUSH, true);
        Bytes out;
        uint64_t consumed = 0;
        fake_inflate(z6.data(), z6.size(), &out, &consumed);
        if (in.second.size() > 1000 && std::string(in.first) != "random")
            CHECK(consumed == 0 && out.empty(), "%s at level 6: consumed %llu", in.first, (unsigned long long)consumed);
    }
    // the hand-over: a prefix, then a level-6 continuation whose matches reach back into the prefix's output
    {
        const Bytes &raw = inputs[4].second;
        Bytes z = deflate_raw(raw, 6, 9, Z_HUFFMAN_ONLY, CH, Z_FULL_FLUSH, false);
        const size_t prefix = z.size();
        Bytes text(raw.end() - 5000, raw.end());
        for (int i = 0; i < 1000; i++) text.insert(text.end(), {'t', 'a', 'i', 'l', ' '});
        const Bytes dict(raw.end() - 32768, raw.end());
        const Bytes rest = deflate_raw(text, 6, 8, Z_DEFAULT_STRATEGY, text.size(), Z_NO_FLUSH, true, &dict);
        z.insert(z.end(), rest.begin(), rest.end());
        Bytes out;
        uint64_t consumed = 0;
        fake_inflate(z.data(), z.size(), &out, &consumed);
        CHECK(consumed == prefix && out == raw, "hand-over: consumed %llu, the prefix is %zu", (unsigned long long)consumed, prefix);
        CHECK(inflate_with_dict(z.data() + consumed, z.size() - consumed, Bytes(out.end() - 32768, out.end()), text.size()) == text, "hand-over: the tail");
    }
    // the limits of one lane's work: 2^20 literals of Huffman blocks, 2^20 blocks in a segment
    {
        const Bytes ones((size_t)P::LITERAL_LIMIT + 100000, 7);
        Bytes z = deflate_raw(Bytes(CH, 9), 6, 9, Z_HUFFMAN_ONLY, CH, Z_FULL_FLUSH, false);
        const size_t prefix = z.size();
        const Bytes run = deflate_raw(ones, 6, 9, Z_HUFFMAN_ONLY, ones.size(), Z_SYNC_FLUSH, false);  // one segment, many blocks
        z.insert(z.end(), run.begin(), run.end());
        Bytes out;
        uint64_t consumed = 0;
        fake_inflate(z.data(), z.size(), &out, &consumed);
        CHECK(consumed == prefix && out == Bytes(CH, 9), "literal limit: consumed %llu, the prefix is %zu", (unsigned long long)consumed, prefix);
        fake_inflate(run.data(), run.size(), &out, &consumed);
        CHECK(consumed == 0 && out.empty(), "literal limit from offset 0: consumed %llu", (unsigned long long)consumed);
        Bytes tiny;  // stored blocks of one byte, byte-aligned: every one is a safe point
        const size_t nblocks = (size_t)P::BLOCK_LIMIT + 10;
        for (size_t i = 0; i < nblocks; i++) tiny.insert(tiny.end(), {0, 1, 0, 0xFE, 0xFF, (uint8_t)i});
        fake_inflate(tiny.data(), tiny.size(), &out, &consumed);
        CHECK(consumed == 6 * P::BLOCK_LIMIT && out.size() == P::BLOCK_LIMIT, "block limit: consumed %llu", (unsigned long long)consumed);
    }
    // hostile headers: every table index stays inside its table whatever the bits say
    for (int t = 0; t < 3000; t++) {
        Bytes junk(1 + rnd() % 300);
        for (auto &v : junk) v = (uint8_t)rnd();
        junk[0] = (uint8_t)((junk[0] & ~7u) | (t % 2 ? 4u : 2u));  // not final, dynamic or fixed
        Bytes out;
        uint64_t consumed = 0;
        fake_inflate(junk.data(), junk.size(), &out, &consumed);
        CHECK(consumed <= junk.size(), "junk");
    }
}

static Bytes read_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    CHECK(f, "%s", path.c_str());
    Bytes b;
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) b.insert(b.end(), buf, buf + got);
    fclose(f);
    return b;
}

// load_unik's device path on the bytes of a file, fake_inflate for the device: "" and the body, or the reason for the host path
static std::string device_gunzip(const Bytes &file, Bytes *header, Bytes *body, uint64_t *upto) {
    unik::GzInput g;
    g.file = file;
    std::string why = g.open_bytes();
    if (!why.empty()) return why;
    Bytes out, tail;
    uint64_t consumed = 0;
    fake_inflate(g.file.data() + g.body_at, g.body_end - g.body_at, &out, &consumed);
    if (consumed == 0) return "nothing consumed";
    const uint64_t total = g.body_total();
    const uint32_t crc = (uint32_t)crc32(g.header_crc, out.data(), (uInt)out.size());
    const size_t n_last = std::min<size_t>(out.size(), 32768);
    why = g.finish(consumed, out.size(), crc, out.data() + (out.size() - n_last), n_last, &tail);
    if (!why.empty()) return why;
    *header = g.header_bytes;
    *body = out;
    body->insert(body->end(), tail.begin(), tail.end());
    CHECK(total == body->size(), "ISIZE says %llu bytes of body, there are %zu", (unsigned long long)total, body->size());
    *upto = g.body_at + consumed;
    return "";
}

static void driver_pieces(const std::string &dir) {
    const size_t CH = 32768;
    Bytes body, tail(13, 0x11);
    for (int i = 0; i < 50000; i++) body.push_back((uint8_t)((i % 7) * (i % 5)));
    const Bytes part1(body.begin(), body.begin() + CH), part2(body.begin() + CH, body.end());
    const Bytes frag1 = deflate_raw(part1, 6, 9, Z_HUFFMAN_ONLY, CH, Z_FULL_FLUSH, false), frag2 = deflate_raw(part2, 6, 9, Z_HUFFMAN_ONLY, CH, Z_FULL_FLUSH, false);
    const uint32_t c1 = (uint32_t)crc32(0, part1.data(), (uInt)part1.size()), c2 = (uint32_t)crc32(0, part2.data(), (uInt)part2.size());
    Bytes good;
    for (int order = 0; order < 4; order++) {
        const std::string path = dir + "/gunzip" + std::to_string(order) + ".unik";
        Bytes want_body;
        std::string desc;
        {
            unik::OutStream os(path, true, order == 3 ? 9 : -1, true);
            unik::Writer w(os, 31, unik::UnikSorted);
            if (order == 3) w.h.description = desc = std::string(300, 'd');
            auto big = [&]() {
                os.write_deflated(frag1.data(), frag1.size(), c1, part1.size());
                os.write_deflated(frag2.data(), frag2.size(), c2, part2.size());
            };
            if (order == 0) { w.write_header(); big(); os.write(tail.data(), tail.size()); want_body = body; want_body.insert(want_body.end(), tail.begin(), tail.end()); }
            if (order == 1) { big(); w.write_header(); }
            if (order == 2) { w.write_header(); os.write(tail.data(), tail.size()); big(); big(); }
            if (order == 3) { w.write_header(); big(); want_body = body; }
            os.close();
        }
        const Bytes file = read_file(path);
        Bytes header, got;
        uint64_t upto = 0;
        const std::string why = device_gunzip(file, &header, &got, &upto);
        if (order == 0 || order == 3) {
            CHECK(why.empty(), "order %d: %s", order, why.c_str());
            CHECK(got == want_body, "order %d: %zu bytes of body, %zu written", order, got.size(), want_body.size());
            CHECK(header.size() == 100 + desc.size() && memcmp(header.data(), ".unikmer", 8) == 0, "order %d: the header", order);
            CHECK(file.size() - upto <= 64, "order %d: the device's part ends %zu bytes in front of the end", order, (size_t)(file.size() - upto));
            unik::Reader r(path);  // and the host path agrees
            Bytes host_body;
            r.read_body(host_body);
            CHECK(host_body == want_body && r.h.description == desc && r.h.k == 31, "order %d: the Reader", order);
            if (order == 0) good = file;
        } else {
            // 1: the body's bytes stand where the header should ("description too long"); 2: the trailing bytes share the header's block
            CHECK(order == 1 ? !why.empty() : why == "the header does not end at a block boundary", "order %d: %s", order, why.c_str());
        }
    }
    Bytes header, got;
    uint64_t upto = 0;
    {   // the refusals, each on the file of order 0 with one thing changed
        Bytes f = good;
        f[3] = 8;
        CHECK(device_gunzip(f, &header, &got, &upto) == "gzip header with FLG != 0", "FLG");
        f = good;
        f[0] = 'x';
        CHECK(device_gunzip(f, &header, &got, &upto) == "not gzip", "magic");
        f = good;
        f[f.size() - 6] ^= 1;
        CHECK(device_gunzip(f, &header, &got, &upto) == "CRC-32 mismatch", "CRC");
        f = good;
        f[f.size() - 2] ^= 1;
        CHECK(device_gunzip(f, &header, &got, &upto) == "size mismatch", "ISIZE");
        f = good;
        f.insert(f.end(), good.begin(), good.end());  // a second member
        CHECK(device_gunzip(f, &header, &got, &upto) == "bytes behind the deflate stream (a second member?)", "second member: %s",
              device_gunzip(f, &header, &got, &upto).c_str());
        f = good;
        f.resize(f.size() - 20);  // truncated
        CHECK(!device_gunzip(f, &header, &got, &upto).empty(), "truncated");
        f = good;
        f[f.size() / 2] ^= 0x20;  // a damaged body: whatever the device makes of it, the trailer does not fit
        CHECK(!device_gunzip(f, &header, &got, &upto).empty(), "damaged body");
        f.assign(good.begin(), good.begin() + 12);
        CHECK(!device_gunzip(f, &header, &got, &upto).empty(), "short");
    }
    {   // a file zlib's own writer made: header and body share a block
        const std::string path = dir + "/host.unik";
        {
            unik::OutStream os(path, true, -1, false);
            unik::Writer w(os, 31, unik::UnikSorted);
            w.write_body(body.data(), body.size());
            os.close();
        }
        const std::string why = device_gunzip(read_file(path), &header, &got, &upto);
        CHECK(why == "the header does not end at a block boundary", "zlib's own file: %s", why.c_str());
        unik::GzInput g;
        CHECK(g.open(dir + "/no such file") == "cannot be opened" && g.open("-") == "stdin", "open");
    }
}

int main(int argc, char **argv) {
    parser_against_zlib();
    if (argc > 1) driver_pieces(argv[1]);
    printf("inflate_units: ok\n");
    return 0;
}
