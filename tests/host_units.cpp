// Stand-alone check of the driver's device-free layer (unikmer_amd/host/base.hpp, seqtext.hpp), built by
// tests/test_host_units_cpu.py with -fsanitize=address,undefined: the flag parser, byte sizes, the FASTA/Q parser (plain
// and gzipped, across its 1 MiB read boundaries), the k-mer text codec, degenerate bases, the rank-order file, the
// nodes.dmp line parser and the two-call idiom.  Expected values are worked out by hand from the rules the code's comments
// state; the k-mer codes were checked once against `unikmer encode -a` / `decode -a`.  The program sets the worker flag, so
// die() throws and the messages can be compared.  usage: host_units <scratch directory>
#include <cstdio>
#include <functional>

#include "seqtext.hpp"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); g_bad++; } } while (0)

// the message die() throws with, "" when fn returns
static string died(const std::function<void()> &fn) {
    try { fn(); } catch (const std::runtime_error &e) { return e.what(); }
    return "";
}

// ---- parse_args ---------------------------------------------------------------------------------------
static Args parse(vector<string> words) {
    vector<char *> argv;
    for (auto &w : words) argv.push_back(&w[0]);
    return parse_args((int)argv.size(), argv.data(), {{'n', "name", true}, {'v', "verb", false}, {'x', "xflag", false}, {'l', "list", true}});
}
static void test_parse_args() {
    typedef vector<string> V;
    CHECK(parse({"--name=value"}).str("name") == "value");
    CHECK(parse({"--name", "value"}).str("name") == "value");
    CHECK(parse({"-nvalue"}).str("name") == "value");
    CHECK(parse({"-n", "value"}).str("name") == "value");
    CHECK(parse({"--name="}).has("name") && parse({"--name="}).str("name", "d") == "");
    CHECK(parse({"-n", "7"}).num("name", 0) == 7 && parse({}).num("name", 3) == 3 && parse({"-n", "0.5"}).real("name", 0) == 0.5);
    for (const V &w : {V{"-vxnfoo", "f"}, V{"-vxn", "foo", "f"}}) {  // bundled short flags, the last one takes the value
        Args a = parse(w);
        CHECK(a.has("verb") && a.has("xflag") && a.str("name") == "foo" && a.files == V{"f"});
    }
    {
        Args a = parse({"-v", "a.unik", "--", "-x", "--name", "b"});  // "--" ends the flags
        CHECK(a.has("verb") && !a.has("xflag") && !a.has("name") && a.files == (V{"a.unik", "-x", "--name", "b"}));
    }
    {
        Args a = parse({"-", "-x", ""});  // a lone "-" (stdin) and an empty word are files
        CHECK(a.has("xflag") && a.files == (V{"-", ""}));
    }
    {
        Args a = parse({"-l", "a,b", "-lc", "--list=d,,e", "--list", "f"});  // a repeated flag, comma lists split, empty pieces dropped
        CHECK(a.list("list") == (V{"a", "b", "c", "d", "e", "f"}) && a.str("list") == "f" && a.list("name").empty());
    }
    CHECK(parse({"-I", "--verbose"}).has("ignore-taxid") && parse({"-I", "--verbose"}).has("verbose"));  // the global flags
    CHECK(died([] { parse({"--nope=3"}); }) == "unknown flag: --nope");
    CHECK(died([] { parse({"-vz"}); }) == "unknown shorthand flag: 'z' in -vz");
    CHECK(died([] { parse({"f", "--name"}); }) == "flag needs an argument: --name");
    CHECK(died([] { parse({"-vn"}); }) == "flag needs an argument: -n");
}

// ---- parse_byte_size ----------------------------------------------------------------------------------
static void test_parse_byte_size() {
    CHECK(parse_byte_size("") == 0);
    CHECK(parse_byte_size(" 12 ") == 12);
    CHECK(parse_byte_size("1K") == 1024);
    CHECK(parse_byte_size("1.5m") == 1572864);
    CHECK(parse_byte_size("2G") == 2147483648LL);
    CHECK(parse_byte_size("7B") == 7);
    CHECK(parse_byte_size("K") == 0);
    CHECK(parse_byte_size("-5") == 0 && parse_byte_size("-5K") == 0);
    CHECK(died([] { parse_byte_size("12x3"); }) == "parsing byte size: invalid byte size: 12x3");
}

// ---- parse_fastx ----------------------------------------------------------------------------------------
typedef vector<std::pair<string, string>> Records;  // (name, sequence)
struct RecordingSink : FastxSink {
    Records recs;
    string skip;            // records of this name are refused
    bool skipping = false, open = false;
    int misuse = 0;         // calls for a refused record, or out of order
    bool begin_record(const string &name) override {
        if (open) misuse++;
        skipping = name == skip;
        if (!skipping) { recs.push_back({name, ""}); open = true; }
        return !skipping;
    }
    void add_seq(const char *p, size_t n) override {
        if (skipping || !open || n == 0) { misuse++; return; }
        recs.back().second.append(p, n);
    }
    void end_record() override {
        if (skipping || !open) misuse++;
        open = false;
    }
};
static void write_file(const string &path, const string &content, bool gz) {
    if (gz) {
        gzFile f = gzopen(path.c_str(), "wb1");
        if (!f || gzwrite(f, content.data(), (unsigned)content.size()) != (int)content.size() || gzclose(f) != Z_OK) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    } else {
        std::ofstream(path, std::ios::binary).write(content.data(), (std::streamsize)content.size());
    }
}
// the content parsed from a plain file and from a gzipped one (through unik::InStream): the same records both times
static void expect_fastx(const string &dir, const string &content, const Records &want, const string &skip = "") {
    for (int gz = 0; gz < 2; gz++) {
        const string path = dir + (gz ? "/in.fx.gz" : "/in.fx");
        write_file(path, content, gz);
        RecordingSink sink;
        sink.skip = skip;
        parse_fastx(path, sink);
        if (sink.recs != want || sink.misuse || sink.open) {
            fprintf(stderr, "parse_fastx (gz=%d, %zu bytes): %zu records, want %zu; misuse %d\n", gz, content.size(), sink.recs.size(), want.size(), sink.misuse);
            for (size_t i = 0; i < sink.recs.size() && i < 8 && sink.recs[i].second.size() < 100; i++) fprintf(stderr, "  [%s] [%s]\n", sink.recs[i].first.c_str(), sink.recs[i].second.c_str());
            g_bad++;
        }
    }
}
static void test_parse_fastx(const string &dir) {
    expect_fastx(dir, ">a desc\nACGT\nTTGA\n>b\nGG\n", {{"a desc", "ACGTTTGA"}, {"b", "GG"}});  // multi-line sequences
    expect_fastx(dir, ">a\nAC GT\tTT\n \t \n G\n", {{"a", "ACGTTTG"}});                            // blanks and tabs inside sequence lines are dropped
    expect_fastx(dir, ">a x\r\nACGT\r\nTT\r\n>b\r\n\r\nG\r\n", {{"a x", "ACGTTT"}, {"b", "G"}});    // CRLF
    expect_fastx(dir, ">a\nACGT\n>b\nTTGA", {{"a", "ACGT"}, {"b", "TTGA"}});                        // no final newline
    expect_fastx(dir, ">a", {{"a", ""}});
    expect_fastx(dir, ">a\n>b\nAC\n>c\n", {{"a", ""}, {"b", "AC"}, {"c", ""}});                     // empty records
    expect_fastx(dir, ">a\nAC\n>skip\nGGGG\nGG\n>c\nTT\n", {{"a", "AC"}, {"c", "TT"}}, "skip");      // a refused record: no add_seq, no end_record
    expect_fastx(dir, ">skip\nGG\n", {}, "skip");
    expect_fastx(dir, "\n\n>a\nAC\n", {{"a", "AC"}});                                                // leading blank lines
    expect_fastx(dir, "", {});
    // FASTQ: a multi-line sequence; the quality is as long as the sequence, so a quality line that begins with '@' is no header
    expect_fastx(dir, "@r1 d\nACGT\nTTGA\n+\n@IIIIIII\n@r2\nGG\n+r2\nII\n", {{"r1 d", "ACGTTTGA"}, {"r2", "GG"}});
    expect_fastx(dir, "@r1\nACGT\nTTGA\n+\nIIII\n@III\n@r2\nG G\n+\n@I", {{"r1", "ACGTTTGA"}, {"r2", "GG"}});
    expect_fastx(dir, "@r1\r\nAC\r\n+\r\n@@\r\n\r\n@skip\r\nTT\r\n+\r\nII\r\n@r3\r\nT\r\n+\r\n@\r\n", {{"r1", "AC"}, {"r3", "T"}}, "skip");
    for (int gz = 0; gz < 2; gz++) {  // a first line that is neither '>' nor '@'; a FASTQ record that does not begin with '@'
        const string path = dir + (gz ? "/bad.fx.gz" : "/bad.fx");
        RecordingSink sink;
        write_file(path, "ACGT\n>a\nAC\n", gz);
        CHECK(died([&] { parse_fastx(path, sink); }) == "invalid FASTA/Q format: " + path);
        write_file(path, "@r1\nAC\n+\nII\nr2\nAC\n+\nII\n", gz);
        CHECK(died([&] { parse_fastx(path, sink); }) == "invalid FASTQ record in " + path);
    }
    CHECK(died([&] { RecordingSink s; parse_fastx(dir + "/no-such-file.fa", s); }) == "fail to open file: " + dir + "/no-such-file.fa");  // (unik::Error)

    // A little over 2 MiB, read in pieces of 1 MiB: the line across the first boundary is cut inside its bases, the line
    // across the second between its '\r' and its '\n'; a header line lies across neither (names would hide a lost byte less well)
    const size_t MiB = 1u << 20;
    string content, seq;
    Records want;
    uint64_t x = 88172645463325252ull;
    auto bases = [&](size_t n) {
        string s(n, 'A');
        for (auto &c : s) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; c = "ACGT"[x >> 62]; }
        return s;
    };
    auto line = [&](size_t n) { const string s = bases(n); content += s + "\r\n"; seq += s; };
    content += ">big one\r\n";
    while (content.size() + 62 < 2 * MiB - 1) line(60);
    line(2 * MiB - 1 - content.size());  // its '\r' is the last byte of the second piece
    while (content.size() < 2 * MiB + 3000) line(60);
    want.push_back({"big one", seq});
    seq.clear();
    content += ">tail\r\n";
    line(17);
    want.push_back({"tail", seq});
    auto is_base = [&](size_t i) { return content[i] != '\r' && content[i] != '\n'; };
    CHECK(is_base(MiB - 1) && is_base(MiB));
    CHECK(content[2 * MiB - 1] == '\r' && content[2 * MiB] == '\n');
    CHECK(content.size() > 2 * MiB && content.size() < 2 * MiB + 4096);
    expect_fastx(dir, content, want);
    // read_fastx: the batch form, with and without names
    write_file(dir + "/b.fa", ">a d\nAC\nG\n>b\nT\n", false);
    SeqBatch b;
    read_fastx(dir + "/b.fa", b, true);
    CHECK(string(b.bases.begin(), b.bases.end()) == "ACGT" && b.off == (vector<u64>{0, 3, 4}) && b.names == (vector<string>{"a d", "b"}));
    read_fastx(dir + "/b.fa", b, false);
    CHECK(b.bases.size() == 8 && b.off == (vector<u64>{0, 3, 4, 7, 8}) && b.names.size() == 2);
}

// ---- k-mer text ---------------------------------------------------------------------------------------------
static void test_kmer_text() {
    u64 c = 0;
    CHECK(encode_kmer("ACGTA", c) && c == 108);  // 00 01 10 11 00
    CHECK(revcomp(108, 5) == 795 && decode_kmer(795, 5) == "TACGT");  // 11 00 01 10 11
    CHECK(encode_kmer("TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTT", c) && c == ~0ull && revcomp(~0ull, 32) == 0);
    CHECK(encode_kmer("u", c) && c == 3 && encode_kmer("N", c) && c == 0);  // U is T; a degenerate base takes its first alternative
    const string pattern = "acgtTGCAggatCCTAacgtTGCAggatCCTA";
    for (int k : {1, 31, 32}) {
        const string s = pattern.substr(0, (size_t)k);
        string upper = s;
        for (auto &ch : upper) ch = (char)toupper((unsigned char)ch);
        CHECK(encode_kmer(s, c) && decode_kmer(c, k) == upper);
        CHECK(k == 32 || c < (1ull << (2 * k)));
        CHECK(revcomp(revcomp(c, k), k) == c);
    }
    for (u64 v : {0ull, 1ull, 27ull, 1023ull}) CHECK(revcomp(revcomp(v, 5), 5) == v);
    c = 77;
    CHECK(!encode_kmer("", c) && !encode_kmer(string(33, 'A'), c) && !encode_kmer("ACGZ", c) && !encode_kmer("AC T", c) && c == 77);
}

// ---- extend_degenerate ----------------------------------------------------------------------------------------
static void test_extend_degenerate() {
    typedef vector<string> V;
    // per base: the first alternative goes to every sequence in place, the further ones are appended, alternative by alternative
    CHECK(extend_degenerate("AN") == (V{"AA", "AC", "AG", "AT"}));
    CHECK(extend_degenerate("RY") == (V{"AC", "GC", "AT", "GT"}));
    CHECK(extend_degenerate("an") == (V{"aa", "ac", "ag", "at"}) && extend_degenerate("aR") == (V{"aA", "aG"}));  // case is kept
    CHECK(extend_degenerate("") == V{""} && extend_degenerate("ACGU") == V{"ACGU"});
    CHECK(extend_degenerate("NNN").size() == 64);
    CHECK(died([] { extend_degenerate("AZ"); }) == "fail to extend degenerate sequence 'AZ': invalid degenerate bases: Z");
}

// ---- read_rank_order_file, parse_two_ids, the small text helpers ---------------------------------------------
static void test_rank_order(const string &dir) {
    const string f = dir + "/ranks.txt";
    // lines in descending order, the LAST line gets order 1; ranks of one line share an order; "!" marks ranks without order
    write_file(f, "# comment\r\n\r\nFamily\r\n  genus , Species,strain,\r\n!No Rank, !Clade\r\n   # indented comment\r\nforma\r\n", false);
    RankOrder ro = read_rank_order_file(f);
    CHECK(ro.order == (std::map<string, int>{{"forma", 1}, {"genus", 2}, {"species", 2}, {"strain", 2}, {"family", 3}}));
    CHECK(ro.noranks == (std::set<string>{"no rank", "clade"}));
    write_file(f, "genus\nfamily,Genus\n", false);
    CHECK(died([&] { read_rank_order_file(f); }) == f + ": duplicated rank: genus");
    write_file(f, "# nothing\n!no rank\n\n", false);
    CHECK(died([&] { read_rank_order_file(f); }) == f + ": no ranks found in file: " + f);
    const string missing = dir + "/no-ranks.txt";
    CHECK(died([&] { read_rank_order_file(missing); }).rfind(missing + ": read rank order list from '" + missing + "': ", 0) == 0);
}
static void test_small_parsers() {
    u32 a = 0, b = 0;
    CHECK(parse_two_ids("9606\t|\t9605\t|\tspecies", a, b) && a == 9606 && b == 9605);
    CHECK(parse_two_ids("12|34", a, b) && a == 12 && b == 34);
    CHECK(!parse_two_ids("9606\t9605\tspecies", a, b));   // no '|'
    CHECK(!parse_two_ids("species\t|\t9605", a, b));      // no leading number
    CHECK(!parse_two_ids("9606\t|\tspecies", a, b) && !parse_two_ids("", a, b) && a == 12 && b == 34);
    string l = "ACGT \r \r";
    trim_line_end(l);
    CHECK(l == "ACGT");
    l = " \tAC\t";
    trim_line_end(l);
    CHECK(l == " \tAC\t");  // only '\r' and blanks, only at the end
    CHECK(trim_space(" \t a b\r\n") == "a b" && trim_space(" \t") == "" && lower_trim("  No Rank\r") == "no rank");
    CHECK(base_of("a/b/c.unik") == "c.unik" && base_of("c") == "c" && base_of("a/") == "");
    CHECK(out_name("-") == "-" && out_name("x") == "x.unik" && out_name("x.unik") == "x.unik" && chunk_file_name("d", 7) == "d/chunk_007.unik");
}
// call_grow / call_sized against a fake entry point that needs `need` entries: -7 stands for UKM_ERR_CAPACITY
static void test_two_call_idiom() {
    const int CAP = -7;
    vector<u64> caps;  // the capacity of every call made
    u64 n = 0;
    auto fake = [&](u64 need, int other) {
        return [&caps, need, other](u64 cap, u64 *m) { caps.push_back(cap); *m = need; return other ? other : cap < need ? -7 : 0; };
    };
    CHECK(call_grow(CAP, 16, &n, fake(16, 0)) == 0 && caps == (vector<u64>{16}) && n == 16);  // the first capacity fits: one call
    caps.clear();
    CHECK(call_grow(CAP, 16, &n, fake(40, 0)) == 0 && caps == (vector<u64>{16, 40}) && n == 40);  // ... does not: again, at the reported count
    caps.clear();
    CHECK(call_sized(CAP, &n, fake(5, 0)) == 0 && caps == (vector<u64>{0, 5}) && n == 5);  // the size query
    caps.clear();
    CHECK(call_sized(CAP, &n, fake(0, 0)) == 0 && caps == (vector<u64>{0}) && n == 0);  // ... that finds nothing to leave: not repeated
    caps.clear();
    u64 grows = 0;  // a call that asks for more every time: the second UKM_ERR_CAPACITY is the result, there is no third call
    CHECK(call_grow(CAP, 1, &n, [&](u64 cap, u64 *m) { caps.push_back(cap); *m = cap + 10; grows++; return -7; }) == CAP && grows == 2);
    CHECK(caps == (vector<u64>{1, 11}) && n == 21);
    caps.clear();
    CHECK(call_grow(CAP, 16, &n, fake(40, -4)) == -4 && caps == (vector<u64>{16}));  // any other code: returned at once
    caps.clear();
    int calls = 0;  // ... and from the second call as well
    CHECK(call_grow(CAP, 16, &n, [&](u64 cap, u64 *m) { caps.push_back(cap); *m = 40; return calls++ ? -10 : -7; }) == -10);
    CHECK(caps == (vector<u64>{16, 40}));
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const string dir = argv[1];
    t_worker_thread = true;  // die() throws instead of ending the process
    try {
        test_parse_args();
        test_parse_byte_size();
        test_parse_fastx(dir);
        test_kmer_text();
        test_extend_degenerate();
        test_rank_order(dir);
        test_small_parsers();
        test_two_call_idiom();
    } catch (const std::exception &e) {
        fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 1;
    }
    if (g_bad) return 1;
    puts("OK");
    return 0;
}
