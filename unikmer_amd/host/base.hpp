// base.hpp — the driver's device-free ground layer: errors and logging, the flag parser, byte sizes, line trimming,
// the two-call idiom of the library's capacity contract, file / directory / path helpers and the two taxonomy text parsers.
// Nothing here includes unikmer_hip.h: the layer compiles beside unik.hpp alone (tests/host_units.cpp runs it under the sanitizers).
#pragma once
#include <dirent.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

using std::string;
using std::vector;
typedef uint64_t u64;
typedef uint32_t u32;

static const string EXT = ".unik";

// ---- errors / logging (util-cli.go:39-44 checkError -> log + os.Exit(-1)) -------------------------
// A worker thread (the FASTA/Q parser of `count`) must not call exit(): atexit handlers and static destructors --
// the HIP runtime's among them -- would run while the main thread is inside HIP calls.  There die() throws; the
// thread's catch hands the message to the main thread, which reports it after join() (round-2 advice).
static thread_local bool t_worker_thread = false;
[[noreturn]] static void die(const char *fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (t_worker_thread) throw std::runtime_error(buf);
    fprintf(stderr, "[ERRO] %s\n", buf);
    // _exit, not exit: a fatal error on the main thread may come while the parser thread of `count` is still filling
    // page-locked chunks; exit() would run atexit handlers and static destructors (the HIP runtime's among them) under it
    fflush(nullptr);
    _exit(255);
}
static bool g_verbose = false;
static void info(const char *fmt, ...) {
    if (!g_verbose) return;
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "[INFO] ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
}

static void warn(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "[WARN] ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
}

// ---- tiny flag parser -----------------------------------------------------------------------------
struct FlagSpec {
    char shortname;  // 0 = none
    const char *longname;
    bool takes_value;
};
struct Args {
    std::map<string, string> val;
    std::set<string> present;
    vector<string> files;
    bool has(const string &k) const { return present.count(k) > 0; }
    string str(const string &k, const string &d = "") const { auto it = val.find(k); return it == val.end() ? d : it->second; }
    long long num(const string &k, long long d) const { auto it = val.find(k); return it == val.end() ? d : atoll(it->second.c_str()); }
    double real(const string &k, double d) const { auto it = val.find(k); return it == val.end() ? d : atof(it->second.c_str()); }
    // every value of a flag that may be given several times, comma-separated lists split (a pflag StringSlice)
    std::map<string, vector<string>> all;
    vector<string> list(const string &k) const {
        vector<string> out;
        auto it = all.find(k);
        if (it == all.end()) return out;
        for (auto &v : it->second) {
            std::istringstream ss(v);
            string piece;
            while (std::getline(ss, piece, ',')) if (!piece.empty()) out.push_back(piece);
        }
        return out;
    }
};

static const vector<FlagSpec> GLOBAL_FLAGS = {
    {'j', "threads", true}, {0, "verbose", false}, {'C', "no-compress", false}, {0, "compression-level", true},
    {'c', "compact", false}, {'i', "infile-list", true}, {0, "max-taxid", true}, {'I', "ignore-taxid", false},
    {0, "data-dir", true}, {0, "skip-flag-check", false}, {0, "skip-file-check", false}, {0, "gpu", true},
    {'h', "help", false},
};

static Args parse_args(int argc, char **argv, vector<FlagSpec> specs) {
    specs.insert(specs.end(), GLOBAL_FLAGS.begin(), GLOBAL_FLAGS.end());
    Args a;
    for (int i = 0; i < argc; i++) {
        string s = argv[i];
        if (s == "-" || s.empty() || s[0] != '-') { a.files.push_back(s); continue; }
        if (s == "--") { for (int j = i + 1; j < argc; j++) a.files.push_back(argv[j]); break; }
        if (s[1] == '-') {
            string name = s.substr(2), value;
            bool has_eq = false;
            size_t eq = name.find('=');
            if (eq != string::npos) { value = name.substr(eq + 1); name = name.substr(0, eq); has_eq = true; }
            const FlagSpec *f = nullptr;
            for (auto &sp : specs) if (name == sp.longname) f = &sp;
            if (!f) die("unknown flag: --%s", name.c_str());
            a.present.insert(f->longname);
            if (f->takes_value) {
                if (!has_eq) { if (i + 1 >= argc) die("flag needs an argument: --%s", name.c_str()); value = argv[++i]; }
                a.val[f->longname] = value; a.all[f->longname].push_back(value);
            }
        } else {
            for (size_t p = 1; p < s.size(); p++) {
                const FlagSpec *f = nullptr;
                for (auto &sp : specs) if (sp.shortname && sp.shortname == s[p]) f = &sp;
                if (!f) die("unknown shorthand flag: '%c' in %s", s[p], s.c_str());
                a.present.insert(f->longname);
                if (f->takes_value) {
                    string value = s.substr(p + 1);
                    if (value.empty()) { if (i + 1 >= argc) die("flag needs an argument: -%c", s[p]); value = argv[++i]; }
                    a.val[f->longname] = value; a.all[f->longname].push_back(value);
                    break;
                }
            }
        }
    }
    return a;
}

// ---- text helpers ---------------------------------------------------------------------------------
// a line of a list file, a query file or k-mer text: '\r' and blanks at its end are dropped
static void trim_line_end(string &line) {
    while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
}
static string trim_space(const string &s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}
static string lower_trim(const string &in) {
    string s = trim_space(in);
    for (auto &ch : s) ch = (char)tolower((unsigned char)ch);
    return s;
}
// util.go:291-335 ParseByteSize: plain number, or B/K/M/G suffix (powers of 1024); "" = 0
static long long parse_byte_size(string v) {
    while (!v.empty() && strchr(" \t\r\n", v.back())) v.pop_back();
    while (!v.empty() && strchr(" \t\r\n", v.front())) v.erase(v.begin());
    if (v.empty()) return 0;
    double unit = 0;
    switch (v.back()) {
    case 'B': case 'b': unit = 1; break;
    case 'K': case 'k': unit = 1 << 10; break;
    case 'M': case 'm': unit = 1 << 20; break;
    case 'G': case 'g': unit = 1 << 30; break;
    default: break;
    }
    if (unit != 0) {
        v.pop_back();
        if (v.empty()) return 0;
    } else {
        unit = 1;
    }
    char *e = nullptr;
    const double x = strtod(v.c_str(), &e);
    if (e == v.c_str() || *e) die("parsing byte size: invalid byte size: %s", v.c_str());
    return x < 0 ? 0 : (long long)(x * unit);
}

// ---- the library's two-call idiom: a call that returns cap_err (UKM_ERR_CAPACITY) has left the count it needs in *n ------
// call(cap, n) sizes the outputs for cap entries and runs the entry point.  call_grow: at a first capacity and, ONLY where that was
// too small, exactly once more at the reported count; the last call's code is the result, a second cap_err included.  call_sized: the
// size query, capacity 0 first (call passes NULL outputs then); a query that succeeds has nothing to leave and is not repeated.
template <class Call> static int call_grow(int cap_err, u64 cap, u64 *n, Call call) {
    const int rc = call(cap, n);
    return rc == cap_err ? call(*n, n) : rc;
}
template <class Call> static int call_sized(int cap_err, u64 *n, Call call) { return call_grow(cap_err, 0, n, call); }

// ---- files, directories, paths --------------------------------------------------------------------
static bool file_exists(const string &p) { struct stat st; return stat(p.c_str(), &st) == 0; }
static bool dir_exists(const string &p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }
static string base_of(const string &p) { size_t s = p.find_last_of('/'); return s == string::npos ? p : p.substr(s + 1); }
static string out_name(const string &prefix) {  // union.go:79-81
    if (prefix == "-") return prefix;
    if (prefix.size() >= EXT.size() && prefix.compare(prefix.size() - EXT.size(), EXT.size(), EXT) == 0) return prefix;
    return prefix + EXT;
}
static string chunk_file_name(const string &dir, int i) {  // util-sort.go:192-194
    char b[64];
    snprintf(b, sizeof b, "chunk_%03d", i);
    return dir + "/" + b + EXT;
}
static vector<string> list_dir(const string &d) {
    vector<string> names;
    DIR *dh = opendir(d.c_str());
    if (!dh) die("check given directory '%s': %s", d.c_str(), strerror(errno));
    while (struct dirent *e = readdir(dh)) { string n = e->d_name; if (n != "." && n != "..") names.push_back(n); }
    closedir(dh);
    std::sort(names.begin(), names.end());
    return names;
}
static void empty_dir(const string &d, const vector<string> &names) {
    for (auto &n : names) if (remove((d + "/" + n).c_str()) != 0) die("fail to remove %s/%s", d.c_str(), n.c_str());
}
// sort.go:113-137 / split.go:108-126: a non-empty directory needs --force; it is then emptied
static void prepare_dir(const string &d, bool force, const char *what) {
    if (dir_exists(d)) {
        vector<string> names = list_dir(d);
        if (!names.empty() && !force) die("%s not empty: %s, choose another one or use --force to overwrite", what, d.c_str());
        empty_dir(d, names);
    } else if (mkdir(d.c_str(), 0777) != 0) {
        // parents (mkdir -p)
        string acc;
        for (size_t i = 0; i <= d.size(); i++)
            if (i == d.size() || d[i] == '/') { acc = d.substr(0, i); if (!acc.empty() && !dir_exists(acc) && mkdir(acc.c_str(), 0777) != 0) die("fail to create directory: %s", acc.c_str()); }
    }
}

// ---- taxonomy text: a nodes.dmp / merged.dmp line, the rank-order file ---------------------------
static bool parse_two_ids(const string &line, u32 &a, u32 &b) {  // "child | parent | ..." (util.go:119-171)
    const char *p = line.c_str();
    char *e = nullptr;
    unsigned long x = strtoul(p, &e, 10);
    if (e == p) return false;
    const char *q = strchr(e, '|');
    if (!q) return false;
    q++;
    unsigned long y = strtoul(q, &e, 10);
    if (e == q) return false;
    a = (u32)x; b = (u32)y;
    return true;
}
// readRankOrderFromFile (rfilter.go:522-580): lines in descending order, the LAST line gets order 1; "!" marks ranks without order
struct RankOrder {
    std::map<string, int> order;
    std::set<string> noranks;
};
static RankOrder read_rank_order_file(const string &file) {
    std::ifstream fh(file);
    if (!fh) die("%s: read rank order list from '%s': %s", file.c_str(), file.c_str(), strerror(errno));
    vector<vector<string>> ranks;
    RankOrder ro;
    string line;
    while (std::getline(fh, line)) {
        const string record = trim_space(line);
        if (record.empty() || record[0] == '#') continue;
        vector<string> items;
        std::istringstream ss(record);
        string item;
        while (std::getline(ss, item, ',')) {
            if (item.empty()) continue;
            item = lower_trim(item);
            if (item.empty()) continue;
            if (item[0] == '!') ro.noranks.insert(item.substr(1));
            else items.push_back(item);
        }
        if (!items.empty()) ranks.push_back(items);
    }
    if (ranks.empty()) die("%s: no ranks found in file: %s", file.c_str(), file.c_str());
    int order = 1;
    for (size_t i = ranks.size(); i-- > 0; order++)
        for (auto &r : ranks[i]) {
            if (ro.order.count(r)) die("%s: duplicated rank: %s", file.c_str(), r.c_str());
            ro.order[r] = order;
        }
    return ro;
}
