// fastx_units.cpp — the FASTA/Q parser of the driver (unikmer_amd/host/seqtext.hpp: parse_fastx) as a stand-alone program,
// built under the address and undefined-behaviour sanitizers by tests/test_fastx_cpu.py.  It needs neither the library nor a
// device.
//   fastx_units parse DIR N        parses DIR/0.in .. DIR/<N-1>.in; DIR/<i>.out gets, for every record, the name, an LF, the
//                                  sequence, an LF (neither can hold an LF) -- or the one line "ERR <the host's message>"
//   fastx_units split DIR FILE...  for every FILE and every split point s: parse_fastx(the first s bytes in memory, the rest as
//                                  a stream through DIR/rest, the format decided by the whole file's first line) must equal the
//                                  one-piece parse of FILE; prints OK
#include <cstdio>
#include <cstring>
#include <string>

#include "seqtext.hpp"

struct TextSink : FastxSink {
    string out;
    bool begin_record(const string &name) override { out += name; out += '\n'; return true; }
    void add_seq(const char *p, size_t n) override { out.append(p, n); }
    void end_record() override { out += '\n'; }
};

static string slurp(const string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    string s;
    char buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}
static void spit(const string &path, const string &s) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || fwrite(s.data(), 1, s.size(), f) != s.size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}
template <class F>
static string run(F &&f) {  // what the sink saw, or ERR and the message the host dies with
    TextSink sink;
    try {
        f(sink);
    } catch (const std::exception &e) {
        return string("ERR ") + e.what() + "\n";
    }
    return sink.out;
}
// parse_fastx's rule for the format: the first line is non-empty and begins with '@'
static bool first_line_is_fastq(const string &text) { return !text.empty() && text[0] == '@'; }

int main(int argc, char **argv) {
    if (argc < 4) return 2;
    t_worker_thread = true;  // die() throws instead of ending the process
    const string mode = argv[1], dir = argv[2];
    if (mode == "parse") {
        const int n = atoi(argv[3]);
        for (int i = 0; i < n; i++) {
            const string in = dir + "/" + std::to_string(i) + ".in";
            spit(dir + "/" + std::to_string(i) + ".out", run([&](FastxSink &s) { parse_fastx(in, s); }));
        }
        printf("OK\n");
        return 0;
    }
    if (mode == "split") {
        int bad = 0;
        for (int a = 3; a < argc; a++) {
            const string file = argv[a], text = slurp(file), rest = dir + "/rest";
            const string want = run([&](FastxSink &s) { parse_fastx(file, s); });
            const bool fastq = first_line_is_fastq(text);
            for (size_t s = 0; s <= text.size(); s++) {
                spit(rest, text.substr(s));
                const string mem = text.substr(0, s);  // a copy of its own size: the sanitizer sees a read past it
                const string got = run([&](FastxSink &sink) {
                    unik::InStream in(rest);
                    parse_fastx(mem.data(), mem.size(), &in, fastq, file, sink);
                });
                if (got != want) {
                    fprintf(stderr, "%s split at %zu:\n%s---- want:\n%s", file.c_str(), s, got.c_str(), want.c_str());
                    bad++;
                }
            }
            // all of it in memory, no stream behind
            const string got = run([&](FastxSink &sink) { parse_fastx(text.data(), text.size(), nullptr, fastq, file, sink); });
            if (got != want) { fprintf(stderr, "%s in memory:\n%s", file.c_str(), got.c_str()); bad++; }
        }
        if (bad) return 1;
        printf("OK\n");
        return 0;
    }
    return 2;
}
