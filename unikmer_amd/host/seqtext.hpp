// seqtext.hpp — device-free sequence text: the k-mer text codec, the FASTA/Q parser, degenerate-base expansion and
// the text streams of the commands that read or print lines.  Like base.hpp it needs unik.hpp (the gzip streams) only.
#pragma once
#include <memory>

#include "base.hpp"
#include "unik.hpp"

// kmers v0.1.0 text <-> code on the host (view / dump / encode / decode only; the throughput
// path is ukm_encode_kmers)
static int base2bit(unsigned char c) {
    switch (c) {
    case 'A': case 'a': case 'N': case 'n': case 'M': case 'm': case 'V': case 'v': case 'H': case 'h':
    case 'R': case 'r': case 'D': case 'd': case 'W': case 'w': return 0;
    case 'C': case 'c': case 'S': case 's': case 'B': case 'b': case 'Y': case 'y': return 1;
    case 'G': case 'g': case 'K': case 'k': return 2;
    case 'T': case 't': case 'U': case 'u': return 3;
    default: return 4;
    }
}
static bool encode_kmer(const string &s, u64 &code) {
    if (s.empty() || s.size() > 32) return false;
    u64 c = 0;
    for (unsigned char ch : s) { int b = base2bit(ch); if (b > 3) return false; c = (c << 2) | (u64)b; }
    code = c;
    return true;
}
static u64 revcomp(u64 code, int k) {
    u64 c = ~code, r = 0;
    for (int i = 0; i < k; i++) { r = (r << 2) | (c & 3); c >>= 2; }
    return r;
}
static string decode_kmer(u64 code, int k) {
    string s((size_t)k, 'A');
    for (int i = k - 1; i >= 0; i--) { s[(size_t)i] = "ACGT"[code & 3]; code >>= 2; }
    return s;
}

// util.go:173-245 extendDegenerateSeq: every sequence a degenerate one stands for, in the reference's order
static vector<string> extend_degenerate(const string &q) {
    static const std::map<char, string> M = {
        {'A', "A"}, {'T', "T"}, {'U', "U"}, {'C', "C"}, {'G', "G"}, {'R', "AG"}, {'Y', "CT"}, {'M', "AC"}, {'K', "GT"}, {'S', "CG"}, {'W', "AT"},
        {'H', "ACT"}, {'B', "CGT"}, {'V', "ACG"}, {'D', "AGT"}, {'N', "ACGT"}, {'a', "a"}, {'t', "t"}, {'u', "u"}, {'c', "c"}, {'g', "g"},
        {'r', "ag"}, {'y', "ct"}, {'m', "ac"}, {'k', "gt"}, {'s', "cg"}, {'w', "at"}, {'h', "act"}, {'b', "cgt"}, {'v', "acg"}, {'d', "agt"},
        {'n', "acgt"}};
    vector<string> seqs = {""};
    for (char base : q) {
        auto it = M.find(base);
        if (it == M.end()) die("fail to extend degenerate sequence '%s': invalid degenerate bases: %c", q.c_str(), base);
        const string &db = it->second;
        vector<string> more;
        for (size_t i = 1; i < db.size(); i++)
            for (auto &sq : seqs) more.push_back(sq + db[i]);
        for (auto &sq : seqs) sq += db[0];
        seqs.insert(seqs.end(), more.begin(), more.end());
    }
    return seqs;
}

// ---- text in and out: a (gzipped) text file in one piece; an output that is gzipped when its name says so ----
static string read_text(const string &file) {
    unik::InStream in(file);
    string text, chunk(1 << 20, '\0');
    for (;;) { size_t got = in.read(&chunk[0], chunk.size()); if (!got) break; text.append(chunk.data(), got); }
    return text;
}
static std::unique_ptr<unik::OutStream> text_out(const string &file) {
    const bool gz = file.size() > 3 && file.compare(file.size() - 3, 3, ".gz") == 0;  // "suffix .gz for gzipped out"
    return std::unique_ptr<unik::OutStream>(new unik::OutStream(file, gz, 6));
}
static void put(unik::OutStream &o, const string &s) { o.write(s.data(), s.size()); }

// ---- FASTA/Q reader (bio/seqio/fastx as used by count.go:289-299) ----------------------------------
struct SeqBatch {
    vector<uint8_t> bases;
    vector<u64> off{0};
    vector<string> names;
};
// FASTA/Q (+gzip) parser (bio/seqio/fastx, count.go:289-299).  The sink decides per record whether it is kept
// (begin_record) and receives the sequence line by line; blanks inside sequence lines are dropped as
// bio/fastx does.
struct FastxSink {
    virtual ~FastxSink() {}
    virtual bool begin_record(const string &name) = 0;  // false: skip this record
    virtual void add_seq(const char *p, size_t n) = 0;
    virtual void end_record() = 0;
};
// The parser proper.  The bytes come from rd(dst, n) -> the number read, 0 at the end; fmt: -1 the first line decides (FASTQ
// iff it is non-empty and begins with '@'), 0 FASTA, 1 FASTQ -- decided by whoever read the start of the file.
template <class Read>
static void parse_fastx_from(Read &&rd, const string &file, FastxSink &sink, int fmt) {
    vector<char> buf(1 << 20);
    bool have = false, keep = false, fastq = fmt == 1;
    int fq_state = 0;  // 0 header, 1 seq, 3 qual
    u64 seq_len = 0, qual_len = 0;
    auto finish = [&]() {
        if (have && keep) sink.end_record();
        have = false;
    };
    auto seq_line = [&](const string &l) -> size_t {
        size_t cnt = 0, s0 = 0;
        for (size_t i = 0; i <= l.size(); i++) {
            if (i == l.size() || l[i] == ' ' || l[i] == '\t') {
                if (i > s0) { if (keep) sink.add_seq(l.data() + s0, i - s0); cnt += i - s0; }
                s0 = i + 1;
            }
        }
        return cnt;
    };
    string carry;
    auto handle = [&](const string &l) {
        if (fastq) {
            if (fq_state == 0) { if (l.empty()) return; if (l[0] != '@') die("invalid FASTQ record in %s", file.c_str()); finish(); have = true; keep = sink.begin_record(l.substr(1)); seq_len = qual_len = 0; fq_state = 1; }
            else if (fq_state == 1) { if (!l.empty() && l[0] == '+') fq_state = 3; else seq_len += seq_line(l); }
            else if (fq_state == 3) { qual_len += l.size(); if (qual_len >= seq_len) fq_state = 0; }
            return;
        }
        if (!l.empty() && l[0] == '>') { finish(); have = true; keep = sink.begin_record(l.substr(1)); return; }
        if (!have) { if (l.empty()) return; die("invalid FASTA/Q format: %s", file.c_str()); }
        seq_line(l);
    };
    bool first = fmt < 0;
    for (;;) {
        size_t n = rd(buf.data(), buf.size());
        if (n == 0) break;
        size_t s0 = 0;
        for (size_t i = 0; i < n; i++) {
            if (buf[i] == '\n') {
                carry.append(buf.data() + s0, i - s0);
                if (!carry.empty() && carry.back() == '\r') carry.pop_back();
                if (first) { first = false; fastq = !carry.empty() && carry[0] == '@'; }
                handle(carry);
                carry.clear();
                s0 = i + 1;
            }
        }
        carry.append(buf.data() + s0, n - s0);
    }
    if (!carry.empty()) { if (first) fastq = carry[0] == '@'; handle(carry); }
    finish();
}
static void parse_fastx(const string &file, FastxSink &sink) {
    unik::InStream in(file);
    parse_fastx_from([&](char *dst, size_t n) { return in.read(dst, n); }, file, sink, -1);
}
// the same from the middle of a file: mem[0, n_mem) -- bytes already in memory, starting where the parser expects a header --
// followed by what `rest` (may be null) still holds, in the format already decided
static void parse_fastx(const char *mem, size_t n_mem, unik::InStream *rest, bool fastq, const string &file, FastxSink &sink) {
    size_t at = 0;
    parse_fastx_from([&](char *dst, size_t n) -> size_t {
        if (at < n_mem) { const size_t got = std::min(n, n_mem - at); memcpy(dst, mem + at, got); at += got; return got; }
        return rest ? rest->read(dst, n) : 0;
    }, file, sink, fastq ? 1 : 0);
}
struct BatchSink : FastxSink {
    SeqBatch &b;
    bool keep_names;
    BatchSink(SeqBatch &bb, bool kn) : b(bb), keep_names(kn) {}
    bool begin_record(const string &name) override { if (keep_names) b.names.push_back(name); return true; }
    void add_seq(const char *p, size_t n) override { b.bases.insert(b.bases.end(), p, p + n); }
    void end_record() override { b.off.push_back(b.bases.size()); }
};
static void read_fastx(const string &file, SeqBatch &b, bool keep_names) {
    BatchSink sink(b, keep_names);
    parse_fastx(file, sink);
}
