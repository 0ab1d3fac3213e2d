// count_pipe_units.cpp — the chunk pipeline of `count` (unikmer_amd/host/count_pipe.hpp) as a stand-alone program with two
// threads, built by tests/test_count_pipe_cpu.py once under the address and undefined-behaviour sanitizers and once under the
// thread sanitizer.  It needs neither the library nor a device: the chunks' memory is malloc / free, the chunk size 64 bytes --
// the smallest shape at which chunk edges, a file's last chunk and the circulation of the three chunks all occur.
//   count_pipe_units DIR    writes its inputs into DIR; one line per case, "OK <case>" or what failed; "OK" at the end
#include <chrono>
#include <cstdio>

#include "count_pipe.hpp"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); g_bad++; } } while (0)

static void *plain_alloc(void *, u64 bytes) { return malloc(bytes); }
static void plain_free(void *, void *p) { free(p); }
static const ChunkAlloc PLAIN = {plain_alloc, plain_free, nullptr};
static const u64 CH = 64;
static void nap() { std::this_thread::sleep_for(std::chrono::milliseconds(1)); }
enum Schedule { FREE_RUNNING, CONSUMER_AHEAD /* the reader naps in front of every read */, READER_AHEAD /* the consumer naps: the reader blocks in get_free */ };

static void spit(const string &path, const string &s) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(s.data(), 1, s.size(), f) != s.size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}
static string letters(size_t n, uint64_t seed) {
    string s(n, 'A');
    uint64_t x = 88172645463325252ull + seed;
    for (auto &c : s) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; c = "ACGT"[x >> 62]; }
    return s;
}

// ---- the raw reader, with a handover at (stop_file, stop_chunk) or none (stop_file -1) -----------------------------------------
struct Inputs {
    vector<string> files, contents;
};
struct Seen { int file; bool first, last, fastq; u64 nb; };
// The consumer is the device thread's loop without a device: the current chunk, the next one fetched in front of its "compute"
// (at the stop only when fetch_nxt), the chunk given back, and at the stop what RawStage::to_host_parser does with the pipe.
static void raw_case(const Inputs &in, int stop_file, int stop_chunk, bool fetch_nxt, Schedule sched) {
    const int before = g_bad;
    ChunkPipe pipe(PLAIN, CH);
    vector<string> got(in.files.size());
    vector<vector<Seen>> seen(in.files.size());
    ReaderThread reader(pipe, [&]() { read_raw_chunks(pipe, in.files, CH, sched == CONSUMER_AHEAD ? nap : nullptr); });
    int hi = pipe.get_full();
    while (hi >= 0) {
        if (sched == READER_AHEAD) nap();
        const HostChunk &h = pipe.chunk(hi);
        const Seen s = {h.file, h.first, h.last, h.fastq, h.nb};
        const bool stop = s.file == stop_file && (int)seen[(size_t)s.file].size() == stop_chunk;
        int nxt = !stop || fetch_nxt ? pipe.get_full() : -1;
        got[(size_t)s.file].append((const char *)h.bases, h.nb);
        seen[(size_t)s.file].push_back(s);
        pipe.put_free(hi);
        if (stop && !s.last) {  // (at a file's last chunk nothing is asked)
            // the reader refills the chunk just given back and blocks in get_free again: it goes on only if take_rest_of
            // wakes it for every chunk it gives back, not just at its end
            if (sched == READER_AHEAD) nap();
            const ChunkPipe::Rest r = pipe.take_rest_of(stop_file, nxt);
            CHECK(r.chunks >= (nxt >= 0 ? 1u : 0u) && r.bytes.size() <= r.chunks * CH);
            nxt = -1;
            got[(size_t)stop_file].append(r.bytes.data(), r.bytes.size());
            CHECK(r.exhausted == (r.stream == nullptr));
            if (r.stream) {  // the parked reader's stream, read to its end by this thread
                CHECK(r.bytes.size() == r.chunks * CH);  // only full chunks lie in front of it
                char buf[50];
                for (;;) { const size_t n = r.stream->read(buf, sizeof buf); got[(size_t)stop_file].append(buf, n); if (n < sizeof buf) break; }
            }
            pipe.release_reader();
        }
        if (nxt < 0) nxt = pipe.get_full();
        hi = nxt;
    }
    reader.join();
    CHECK(pipe.error().empty());
    CHECK(pipe.idle());  // nothing queued, every chunk back exactly once
    for (size_t f = 0; f < in.files.size(); f++) {
        const string &want = in.contents[f];
        CHECK(got[f] == want);  // the chunks, take_rest_of's bytes and the stream: the file, once and in order
        const size_t nchunks = want.size() / CH + 1;  // the last chunk is the first short read
        const bool handed = (int)f == stop_file && (size_t)stop_chunk + 1 < nchunks;
        CHECK(seen[f].size() == (handed ? (size_t)stop_chunk + 1 : nchunks));
        for (size_t c = 0; c < seen[f].size(); c++) {
            const Seen &s = seen[f][c];
            CHECK(s.file == (int)f && s.nb == std::min<u64>(CH, want.size() - c * CH));
            CHECK(s.first == (c == 0) && s.last == (c + 1 == nchunks) && s.fastq == (!want.empty() && want[0] == '@'));
        }
    }
    if (g_bad != before) fprintf(stderr, "  in raw_case(stop_file %d, stop_chunk %d, fetch_nxt %d, schedule %d)\n", stop_file, stop_chunk, (int)fetch_nxt, (int)sched);
}
static void test_raw_reader(const Inputs &in) {
    for (Schedule s : {FREE_RUNNING, CONSUMER_AHEAD, READER_AHEAD}) raw_case(in, -1, 0, true, s);
}
static void test_handover_everywhere(const Inputs &in) {
    for (size_t f = 0; f < in.files.size(); f++)
        for (size_t c = 0; c < in.contents[f].size() / CH + 1; c++)
            for (int fetch = 0; fetch < 2; fetch++)
                for (Schedule s : {CONSUMER_AHEAD, READER_AHEAD}) raw_case(in, (int)f, (int)c, fetch != 0, s);
}

// ---- the double-buffered loop: the order of a stage's calls ------------------------------------------------------------------------
struct LoggingStage {
    ChunkPipe &pipe;
    string log;
    int held[2] = {-1, -1}, uploads = 0;
    void fence() { log += "f "; }
    void upload(int s, int hi) {
        CHECK(held[s] < 0);
        held[s] = hi;
        log += "u" + std::to_string(s) + ":" + std::to_string(uploads++) + " ";
    }
    void compute(int s, int o, int &nxt) {
        CHECK(o == (s ^ 1) && held[s] >= 0 && held[o] == nxt);  // the next chunk is on its way before this one is computed
        log += "c" + std::to_string(s) + " ";
        pipe.put_free(held[s]);
        held[s] = -1;
    }
};
static void test_loop(const Inputs &in) {
    ChunkPipe pipe(PLAIN, CH);
    const vector<string> one = {in.files[0]};  // 203 bytes: four chunks
    ReaderThread reader(pipe, [&]() { read_raw_chunks(pipe, one, CH); });
    LoggingStage stage{pipe};
    run_double_buffered(pipe, stage);
    reader.join();
    CHECK(stage.log == "u0:0 f u1:1 c0 f u0:2 c1 f u1:3 c0 f c1 ");
    CHECK(pipe.idle() && pipe.error().empty());
    ChunkPipe none(PLAIN, CH);  // no chunk at all: no call
    ReaderThread idle_reader(none, []() {});
    LoggingStage unused{none};
    run_double_buffered(none, unused);
    CHECK(unused.log.empty() && none.idle());
}

// ---- the parsing reader -------------------------------------------------------------------------------------------------------
struct Parsed {
    vector<uint8_t> bases;
    vector<u64> off{0};
    vector<u32> wtax;
    size_t chunks = 0;
};
static Parsed through_the_pipe(const vector<string> &files, const RecordRules &rules) {
    Parsed p;
    ChunkPipe pipe(PLAIN, CH);  // (a record longer than a chunk grows the chunk's buffer)
    ReaderThread reader(pipe, [&]() { read_parsed_chunks(pipe, files, CH, rules, nullptr); });
    for (int i; (i = pipe.get_full()) >= 0; pipe.put_free(i)) {
        const HostChunk &h = pipe.chunk(i);
        CHECK(h.off.size() > 1 && h.off[0] == 0 && h.off.back() == h.nb);
        for (size_t r = 1; r < h.off.size(); r++) p.off.push_back(p.bases.size() + h.off[r]);
        p.bases.insert(p.bases.end(), h.bases, h.bases + h.nb);
        p.wtax.insert(p.wtax.end(), h.wtax.begin(), h.wtax.end());
        p.chunks++;
    }
    reader.join();
    CHECK(pipe.error().empty() && !pipe.idle());  // (the sink ends holding the chunk it would have filled next)
    return p;
}
static void test_parsing_reader(const string &dir) {
    // records shorter than, equal to and longer than a chunk, an empty one, one the name filter leaves out
    const string text = ">short taxid=7\nACGTAC\n>equal taxid=9\n" + letters(CH, 1) + "\n>long taxid=11\n" + letters(80, 2) + "\n" + letters(70, 3) +
                        "\n>empty taxid=5\n>skip me taxid=3\nGGGGGGGG\n>tiny taxid=13\nACG\n>after taxid=15\n" + letters(40, 4) + "\n";
    const string file = dir + "/records.fa", second = dir + "/second.fa";
    spit(file, text);
    spit(second, ">second taxid=2\n" + letters(30, 5) + "\n");
    const std::regex skip("^SKIP", std::regex::icase), tax_re("taxid=(\\d+)");
    const int k = 5;
    // what read_fastx gives on the whole files, the filter and the taxid rule applied record by record
    Parsed want;
    vector<u32> want_circular;
    for (auto &f : {file, second}) {
        SeqBatch b;
        read_fastx(f, b, true);
        for (size_t r = 0; r < b.names.size(); r++) {
            if (std::regex_search(b.names[r], skip)) continue;
            want.bases.insert(want.bases.end(), b.bases.begin() + (long)b.off[r], b.bases.begin() + (long)b.off[r + 1]);
            want.off.push_back(want.bases.size());
            const u64 len = b.off[r + 1] - b.off[r];
            std::smatch m;
            CHECK(std::regex_search(b.names[r], m, tax_re));
            if (len >= (u64)k) {  // a record too short for a window has no taxid to give
                want.wtax.insert(want.wtax.end(), len - k + 1, (u32)atoi(m[1].str().c_str()));
                want_circular.insert(want_circular.end(), len, (u32)atoi(m[1].str().c_str()));
            }
        }
    }
    CHECK(want.off.size() == 1 + 7);
    RecordRules rules;
    rules.skip_name = &skip;
    Parsed got = through_the_pipe({file, second}, rules);
    CHECK(got.bases == want.bases && got.off == want.off && got.wtax.empty() && got.chunks >= 3);
    rules.tax_re = &tax_re;
    rules.k = k;
    got = through_the_pipe({file, second}, rules);
    CHECK(got.bases == want.bases && got.off == want.off && got.wtax == want.wtax);
    rules.circular = true;
    got = through_the_pipe({file, second}, rules);
    CHECK(got.bases == want.bases && got.off == want.off && got.wtax == want_circular);
}
// a text parse_fastx dies on: the message is in the error slot and get_full ends without blocking
static void test_reader_error(const string &dir) {
    const string file = dir + "/bad.fa";
    spit(file, ">a\n" + letters(100, 6) + "\n>b\nAC\n");
    const string garbage = dir + "/garbage.fa";
    spit(garbage, "ACGT\n>a\nAC\n");
    ChunkPipe pipe(PLAIN, CH);
    ReaderThread reader(pipe, [&]() { read_parsed_chunks(pipe, {file, garbage}, CH, RecordRules(), nullptr); });
    size_t chunks = 0;
    for (int i; (i = pipe.get_full()) >= 0; pipe.put_free(i)) chunks++;
    CHECK(chunks == 1);  // the record that filled a chunk in front of the error
    CHECK(pipe.get_full() == -1);
    reader.join();
    CHECK(pipe.error() == "invalid FASTA/Q format: " + garbage);
    // the same for the raw reader and a file that is not there
    ChunkPipe raw(PLAIN, CH);
    const vector<string> missing = {dir + "/no-such-file.fa"};
    ReaderThread raw_reader(raw, [&]() { read_raw_chunks(raw, missing, CH); });
    CHECK(raw.get_full() == -1);
    raw_reader.join();
    CHECK(raw.error() == "fail to open file: " + missing[0] && raw.idle());
}
// the consumer leaves while the reader waits for a free chunk: the reader's destructor wakes it and joins
static void test_abandon(const Inputs &in) {
    ChunkPipe pipe(PLAIN, CH);
    {
        ReaderThread reader(pipe, [&]() { read_raw_chunks(pipe, in.files, CH); });
        CHECK(pipe.get_full() >= 0);  // taken and never given back
    }
    CHECK(pipe.error() == "count: the chunk pipeline was abandoned" && pipe.get_full() >= 0);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const string dir = argv[1];
    t_worker_thread = true;  // die() throws instead of ending the process
    // a few hundred bytes that are no multiple of the chunk size, an empty file, exactly one chunk; one file is FASTQ by its first byte
    Inputs in;
    const size_t sizes[] = {203, 0, CH, 330, 150};
    for (size_t f = 0; f < 5; f++) {
        in.files.push_back(dir + "/raw" + std::to_string(f));
        in.contents.push_back((f == 3 && sizes[f] ? "@" : "") + letters(sizes[f] - (f == 3 ? 1 : 0), 10 + f));
        spit(in.files.back(), in.contents.back());
    }
    struct { const char *name; std::function<void()> run; } cases[] = {
        {"raw reader", [&] { test_raw_reader(in); }},
        {"handover at every position", [&] { test_handover_everywhere(in); }},
        {"double-buffered loop", [&] { test_loop(in); }},
        {"parsing reader", [&] { test_parsing_reader(dir); }},
        {"reader errors", [&] { test_reader_error(dir); }},
        {"abandoned pipeline", [&] { test_abandon(in); }},
    };
    for (auto &c : cases) {
        const int before = g_bad;
        try {
            c.run();
        } catch (const std::exception &e) {
            fprintf(stderr, "unexpected exception: %s\n", e.what());
            g_bad++;
        }
        printf("%s %s\n", g_bad == before ? "OK" : "FAILED", c.name);
        fflush(stdout);
    }
    if (g_bad) return 1;
    puts("OK");
    return 0;
}
