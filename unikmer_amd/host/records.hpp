// records.hpp — the record layer: everything that moves records between .unik files, host vectors and library calls.
// Options, the device context, one loaded file, THE input loader (all inputs checked against the first, in the three
// shapes commands want them), the writers, and the steps several commands share: stream pointers, a taxid for every
// record, sort-then-unique, the per-file selection loop, the output header's flags.
#pragma once
#include "../../include/unikmer_hip.h"
#include "seqtext.hpp"

// ---- options shared by all commands (util.go:52-109) -----------------------------------------------
// Whether load_unik / write_unik / write_following decode and encode bodies on the device when nothing is said in the
// environment: yes -- `union` of two files of 1e8 records takes 3.4 s against the host codec's 4.6 s.
// UNIKMER_HOST_CODEC=1 keeps the host codec of unik.hpp everywhere (the comparison path of the tests and of the measurement),
// UNIKMER_DEVICE_CODEC=1 asks for the device codec whatever the default.
static const bool DEVICE_CODEC_DEFAULT = true;
// The same switch for the text of `view` (ukm_view) and `dump` (ukm_dump), one default per command;
// UNIKMER_HOST_TEXT=1 keeps the host loops of cmd_cpu.hpp, UNIKMER_DEVICE_TEXT=1 asks for the device path in both.
static const bool DEVICE_VIEW_DEFAULT = false, DEVICE_DUMP_DEFAULT = true;
// And for the gzip of a .unik OUTPUT (write_unik, write_following): the body is deflated on the device (ukm_deflate: Huffman
// coding in independent chunks) and only the compressed bytes are downloaded, where the device codec is on.
// UNIKMER_DEVICE_GZIP=1 asks for it, UNIKMER_HOST_GZIP=1 keeps zlib everywhere.  --compression-level 0, text outputs and the
// commands without a device (num, info, concat, head) stay on zlib whatever is said.
static const bool DEVICE_GZIP_DEFAULT = false;
// And for the gzip of a .unik INPUT (load_unik): zlib reads the header, the compressed body is uploaded and inflated on the
// device (ukm_inflate) straight into the buffer ukm_unik_decode reads, where the device codec is on and the file is a regular
// gzip file whose body is Huffman-only blocks -- what the device gzip above writes.  Any other file goes
// through zlib as before.  UNIKMER_DEVICE_GUNZIP=1 asks for it, UNIKMER_HOST_GUNZIP=1 keeps zlib everywhere; stdin and the
// commands without a device stay on zlib whatever is said.  UNIKMER_GUNZIP_REPORT=1: one line per input file on stderr,
// "gunzip: <path>: device <bytes of the file the device's part ends at> of <file size> bytes" or "... host (<reason>)".
static const bool DEVICE_GUNZIP_DEFAULT = false;
// And for the FASTA/Q input of `count` (cmd_count.hpp, count_pipe.hpp): the reader thread hands raw (inflated) bytes on, ukm_fastx parses
// them where the encode kernels read, and what is outside its grammar goes to parse_fastx from the byte it names (DESIGN.md
// 4.21).  UNIKMER_DEVICE_FASTX=1 asks for it, UNIKMER_HOST_FASTX=1 keeps the host parser; -B and -T need a name per record and
// stay with the host parser whatever is said.  UNIKMER_FASTX_REPORT=1: one line per input file on stderr,
// "fastx: <path>: device, <N> chunk(s)[, host from byte <B> (grammar)]" or "fastx: <path>: host (<reason>)".
static const bool DEVICE_FASTX_DEFAULT = false;
struct Options {
    bool compress = true, compact = false, ignore_taxid = false, skip_file_check = false;
    int level = -1, gpu = 0;
    bool device_codec = DEVICE_CODEC_DEFAULT;  // .unik bodies through ukm_unik_decode / ukm_unik_encode (load_unik, write_unik)
    bool device_view = DEVICE_VIEW_DEFAULT, device_dump = DEVICE_DUMP_DEFAULT;  // view / dump text through ukm_view / ukm_dump
    bool device_gzip = DEVICE_GZIP_DEFAULT;    // compressed .unik outputs through ukm_deflate (write_unik, write_following)
    bool device_gunzip = DEVICE_GUNZIP_DEFAULT, gunzip_report = false;  // gzip .unik inputs through ukm_inflate (load_unik)
    bool device_fastx = DEVICE_FASTX_DEFAULT, fastx_report = false;        // the input of count through ukm_fastx (count_on_device)
    u64 chunk_bytes = 32u << 20;  // UNIKMER_CHUNK_MB (default 32, at least 1): the bytes of a chunk of count's pipeline
    u32 max_taxid = 0xFFFFFFFFu;
    string data_dir;
};
// One switch of the environment: UNIKMER_DEVICE_<x>=1 turns it on, UNIKMER_HOST_<x>=1 turns it off and wins; where neither
// is said every flag of the switch keeps its default.  report: UNIKMER_<x>_REPORT=1.
static void env_switch(const string &x, std::initializer_list<bool *> flags, bool *report = nullptr) {
    auto is_1 = [](const string &name) { const char *v = getenv(name.c_str()); return v && v[0] == '1'; };
    if (is_1("UNIKMER_DEVICE_" + x)) for (bool *f : flags) *f = true;
    if (is_1("UNIKMER_HOST_" + x)) for (bool *f : flags) *f = false;
    if (report) *report = is_1("UNIKMER_" + x + "_REPORT");
}
static Options get_options(const Args &a) {
    Options o;
    g_verbose = a.has("verbose");
    o.compress = !a.has("no-compress");
    o.level = (int)a.num("compression-level", -1);
    o.compact = a.has("compact");
    o.ignore_taxid = a.has("ignore-taxid");
    o.skip_file_check = a.has("skip-file-check");
    o.max_taxid = (u32)a.num("max-taxid", 0xFFFFFFFFLL);
    const char *env = getenv("UNIKMER_DB");  // util.go:75-83
    const char *home = getenv("HOME");
    o.data_dir = a.has("data-dir") ? a.str("data-dir") : (env ? string(env) : (string(home ? home : ".") + "/.unikmer"));
    const char *g = getenv("UNIKMER_GPU");
    o.gpu = (int)a.num("gpu", g ? atoi(g) : 0);
    env_switch("CODEC", {&o.device_codec});
    env_switch("TEXT", {&o.device_view, &o.device_dump});
    env_switch("GZIP", {&o.device_gzip});
    env_switch("GUNZIP", {&o.device_gunzip}, &o.gunzip_report);
    env_switch("FASTX", {&o.device_fastx}, &o.fastx_report);
    const char *mb = getenv("UNIKMER_CHUNK_MB");
    o.chunk_bytes = (u64)(mb ? std::max(1, atoi(mb)) : 32) << 20;
    return o;
}
// util-cli.go:192-264 : files from the command line plus the optional list file; "-" = stdin
static vector<string> get_files(const Args &a, const Options &o, bool allow_stdin_default = true) {
    vector<string> files = a.files;
    if (a.has("infile-list")) {
        std::ifstream fh(a.str("infile-list"));
        if (!fh) die("fail to read file list: %s", a.str("infile-list").c_str());
        string line;
        while (std::getline(fh, line)) {
            trim_line_end(line);
            if (!line.empty()) files.push_back(line);
        }
    }
    if (files.empty() && allow_stdin_default) files.push_back("-");
    if (!o.skip_file_check)
        for (auto &f : files)
            if (f != "-" && !file_exists(f)) die("file does not exist: %s", f.c_str());
    return files;
}

// ---- GPU context + device buffers ---------------------------------------------------------------
// the first context of the process that is still alive: the one the .unik codec borrows (codec_ctx)
static ukm_ctx *g_first_ctx = nullptr;
struct Gpu {
    ukm_ctx *c = nullptr;
    explicit Gpu(int device) {
        if (ukm_ctx_create(device, &c) != UKM_OK) die("%s", ukm_last_error());
        if (!g_first_ctx) g_first_ctx = c;
    }
    ~Gpu() {
        if (g_first_ctx == c) g_first_ctx = nullptr;
        if (c) ukm_ctx_destroy(c);
    }
};
static void ck(int rc) { if (rc != UKM_OK) die("%s", ukm_last_error()); }
struct DevMem {
    ukm_ctx *c;
    void *p = nullptr;
    DevMem(ukm_ctx *ctx, u64 bytes) : c(ctx) { ck(ukm_dev_alloc(c, bytes ? bytes : 8, &p)); }
    ~DevMem() { if (p) ukm_dev_free(c, p); }
    DevMem(const DevMem &) = delete;
};
// Device memory that grows.  ensure(want): at least `want` bytes, the contents dropped -- the old memory is freed first and
// want + want / 8 bytes are allocated (a buffer refilled chunk after chunk).  ensure(want, keep), keep > 0: the first `keep`
// bytes stay -- at least twice the old size is allocated and they are copied (an array that is appended to).
struct DevBuf {
    ukm_ctx *c;
    uint8_t *p = nullptr;
    u64 cap = 0;
    explicit DevBuf(ukm_ctx *ctx) : c(ctx) {}
    DevBuf(ukm_ctx *ctx, u64 bytes) : c(ctx), cap(bytes) { void *q = nullptr; ck(ukm_dev_alloc(c, bytes, &q)); p = (uint8_t *)q; }  // exactly `bytes`
    ~DevBuf() { if (p) ukm_dev_free(c, p); }
    DevBuf(const DevBuf &) = delete;
    void swap(DevBuf &o) { std::swap(c, o.c); std::swap(p, o.p); std::swap(cap, o.cap); }
    template <class T> T *as() const { return (T *)p; }
    void ensure(u64 want, u64 keep = 0) {
        if (want <= cap) return;
        if (!keep) DevBuf(c).swap(*this);
        DevBuf grown(c, keep ? std::max<u64>(want, cap * 2) : want + want / 8);
        if (keep) ck(ukm_copy(c, grown.p, p, keep));
        swap(grown);
    }
};
// page-locked host memory of a context as the two plain functions of count_pipe.hpp's ChunkAlloc (the cookie is the context)
static void *pinned_alloc(void *ctx, u64 bytes) { void *p = nullptr; ck(ukm_host_alloc((ukm_ctx *)ctx, bytes, &p)); return p; }
static void pinned_free(void *ctx, void *p) { ukm_host_free((ukm_ctx *)ctx, p); }

// The context the device codec runs on: the command's own where it has made one already, else one made here on first use and
// kept for the process (*own: the caller trims its workspace after the call, the command's context will want the memory).
// nullptr: the host codec is to be used -- it was asked for, or this machine has no device (the command then fails where
// it needs one itself, or needs none: empty inputs).
static ukm_ctx *codec_ctx(const Options &o, bool *own) {
    *own = false;
    if (!o.device_codec) return nullptr;
    if (g_first_ctx) return g_first_ctx;
    static ukm_ctx *mine = nullptr;
    static bool tried = false;
    if (!tried) {
        tried = true;
        if (ukm_ctx_create(o.gpu, &mine) != UKM_OK) mine = nullptr;
    }
    *own = mine != nullptr;
    return mine;
}

// The context ukm_view / ukm_dump run on: codec_ctx's, whatever is said about the codec.  nullptr: the host loops run -- they
// were asked for, or this machine has no device (view and dump stay usable there).
static ukm_ctx *text_ctx(const Options &o, bool wanted, bool *own) {
    *own = false;
    if (!wanted) return nullptr;
    Options oc = o;
    oc.device_codec = true;
    return codec_ctx(oc, own);
}

// ---- taxonomy (util.go:119-171): nodes.dmp (+ merged.dmp) -> ukm_taxonomy_load ---------------------
static u32 load_taxonomy(Gpu &g, const Options &o) {
    const string nodes = o.data_dir + "/nodes.dmp", merged = o.data_dir + "/merged.dmp";
    if (!file_exists(nodes))
        die("taxonomy file not found: %s (set --data-dir or UNIKMER_DB)", nodes.c_str());
    info("loading Taxonomy from: %s", o.data_dir.c_str());
    vector<u32> child, parent, mo, mn;
    std::ifstream fh(nodes);
    string line;
    u32 a, b;
    while (std::getline(fh, line)) if (parse_two_ids(line, a, b)) { child.push_back(a); parent.push_back(b); }
    if (file_exists(merged)) {
        std::ifstream mh(merged);
        while (std::getline(mh, line)) if (parse_two_ids(line, a, b)) { mo.push_back(a); mn.push_back(b); }
    }
    info("%zu nodes loaded, %zu merged nodes loaded", child.size(), mo.size());
    ck(ukm_taxonomy_load(g.c, child.data(), parent.data(), child.size(), mo.empty() ? nullptr : mo.data(),
                         mn.empty() ? nullptr : mn.data(), mo.size()));
    u32 mx = 0;
    ck(ukm_taxonomy_max_taxid(g.c, &mx));
    return mx;  // util.go:169: opt.MaxTaxid follows the taxonomy
}

// ---- one loaded .unik file ---------------------------------------------------------------------------
struct Loaded {
    unik::Header h;
    vector<u64> codes;
    vector<u32> taxids;  // filled when has_taxid and the records carry their own (UnikIncludeTaxID)
    // the header's global taxid (`count -t`, count.go:466-468) when the records carry none: unik.Reader hands it out with
    // every record; the library takes it as ONE number per file (ukm_*_ft) -- nothing is expanded on the host
    u32 file_taxid = 0;
    bool has_taxid = false;
    bool per_record() const { return has_taxid && h.is_include_taxid(); }
};
// the records of a body in one piece (host or device memory), decoded by ukm_unik_decode into L's host vectors (a
// device-resident Loaded is the follow-up)
static void decode_body(ukm_ctx *c, const string &file, const unik::Header &h, const uint8_t *body, u64 nbody, Loaded &L) {
    const bool tx = L.per_record();
    u64 n = 0, guess = h.number == ~0ull ? 0 : std::min<u64>(h.number, nbody);  // (a record takes more than a byte)
    const int rc = call_grow(UKM_ERR_CAPACITY, guess, &n, [&](u64 cap, u64 *m) {
        L.codes.resize(cap); if (tx) L.taxids.resize(cap);
        return ukm_unik_decode(c, body, nbody, h.k, h.flag, h.taxid_bytes, cap ? L.codes.data() : nullptr,
                               cap && tx ? L.taxids.data() : nullptr, cap, m);
    });
    if (rc == UKM_ERR_FORMAT)  // the Reader's own words
        throw unik::Error(string(strstr(ukm_last_error(), "truncated record") ? "truncated record: " : "unexpected EOF: ") + file);
    ck(rc);
    L.codes.resize(n); if (tx) L.taxids.resize(n);
}
static bool codec_takes(const unik::Header &h) {  // (no file outside is written; the Reader's arithmetic decides)
    return !(h.is_compact() && !h.is_sorted() && (h.k < 1 || h.k > 32));
}
// The device gunzip path: false with the reason in `why` where the file is to go through zlib.  The inflated body never
// crosses to the host: ukm_inflate writes it into the device buffer ukm_unik_decode reads.
static bool load_unik_device_gunzip(const string &file, const Options &o, ukm_ctx *c, Loaded &L, string &why, u64 *upto, u64 *size) {
    unik::GzInput g;
    why = g.open(file);
    if (!why.empty()) return false;
    if (!codec_takes(g.h)) { why = "a layout the device codec does not take"; return false; }
    const u64 n = g.body_end - g.body_at;
    u64 cap = g.body_total();
    if (!cap) { why = "nothing to inflate, or a size the trailer cannot mean"; return false; }
    std::unique_ptr<DevMem> body(new DevMem(c, cap));
    u64 n_out = 0, consumed = 0;
    uint32_t crc = g.header_crc;
    {
        DevMem src(c, n);
        ck(ukm_copy(c, src.p, g.file.data() + g.body_at, n));
        int rc = ukm_inflate(c, (const uint8_t *)src.p, n, 0, (uint8_t *)body->p, cap, &n_out, &consumed, &crc);
        if (rc == UKM_ERR_CAPACITY) {  // ISIZE is the size modulo 2^32
            body.reset();
            cap = n_out;
            body.reset(new DevMem(c, cap));
            crc = g.header_crc;
            rc = ukm_inflate(c, (const uint8_t *)src.p, n, 0, (uint8_t *)body->p, cap, &n_out, &consumed, &crc);
        }
        ck(rc);
    }
    if (consumed == 0) { why = "no block the device takes (a stream with matches)"; return false; }
    vector<uint8_t> last((size_t)std::min<u64>(n_out, 32768)), tail;
    if (!last.empty()) ck(ukm_copy(c, last.data(), (const uint8_t *)body->p + (n_out - last.size()), last.size()));
    why = g.finish(consumed, n_out, crc, last.data(), last.size(), &tail);
    if (!why.empty()) return false;
    if (n_out + tail.size() > cap) {
        std::unique_ptr<DevMem> more(new DevMem(c, n_out + tail.size()));
        if (n_out) ck(ukm_copy(c, more->p, body->p, n_out));
        body.swap(more);
    }
    if (!tail.empty()) ck(ukm_copy(c, (uint8_t *)body->p + n_out, tail.data(), tail.size()));
    L.h = g.h;
    L.has_taxid = !o.ignore_taxid && g.h.has_taxid_info();
    *upto = g.body_at + consumed;
    *size = g.file.size();
    vector<uint8_t>().swap(g.file);
    decode_body(c, file, g.h, (const uint8_t *)body->p, n_out + tail.size(), L);
    return true;
}
static Loaded load_unik(const string &file, const Options &o) {
    bool own = false;
    string why = "device gunzip is off";
    if (o.device_gunzip) {  // (only here is a context made before the file has been looked at)
        Loaded L;
        u64 upto = 0, size = 0;
        ukm_ctx *c = codec_ctx(o, &own);
        if (!c) why = "no device codec";
        else if (load_unik_device_gunzip(file, o, c, L, why, &upto, &size)) {
            if (o.gunzip_report) fprintf(stderr, "gunzip: %s: device %llu of %llu bytes\n", file.c_str(), (unsigned long long)upto, (unsigned long long)size);
            if (own) ck(ukm_ctx_trim(c));
            if (L.has_taxid && !L.per_record()) L.file_taxid = L.h.global_taxid;
            return L;
        }
    }
    if (o.gunzip_report) fprintf(stderr, "gunzip: %s: host (%s)\n", file.c_str(), why.c_str());
    unik::Reader r(file);
    Loaded L;
    L.h = r.h;
    L.has_taxid = !o.ignore_taxid && r.h.has_taxid_info();
    ukm_ctx *c = codec_ctx(o, &own);
    if (c && !codec_takes(r.h)) c = nullptr;
    if (c) {
        vector<uint8_t> body;
        r.read_body(body);
        decode_body(c, file, r.h, body.data(), body.size(), L);
        if (own) ck(ukm_ctx_trim(c));
    } else {
        r.read_all(L.codes, L.per_record() ? &L.taxids : nullptr);
    }
    if (L.has_taxid && !L.per_record()) L.file_taxid = r.h.global_taxid;
    return L;
}
// A taxid for each of n records of L: those of `own` from index `from` on where the records carry their own (L's column, or
// a selection's), else the file's one taxid n times.
static void append_taxids(const Loaded &L, const vector<u32> &own, u64 from, u64 n, vector<u32> &dst) {
    if (L.per_record()) dst.insert(dst.end(), own.begin() + (long)from, own.begin() + (long)(from + n));
    else dst.insert(dst.end(), (size_t)n, L.file_taxid);
}
static void check_compat(const unik::Header &a, const unik::Header &b, const string &file) {  // util-binary-file.go:31-44
    if (a.k != b.k) die("k-mer length not consistent (%d != %d), please check with \"unikmer stats\": %s", a.k, b.k, file.c_str());
    if (a.is_canonical() != b.is_canonical()) die("'canonical' flags not consistent, please check with \"unikmer stats\": %s", file.c_str());
    if (a.is_hashed() != b.is_hashed()) die("'hashed' flags not consistent, please check with \"unikmer stats\": %s", file.c_str());
    if (a.is_scaled() != b.is_scaled()) die("'scaled' flags not consistent, please check with \"unikmer stats\": %s", file.c_str());
}

// ---- the input loader: every input, checked against the first ----------------------------------------
// What a command asks of its inputs.  The messages are the command's own: where two commands word one condition
// differently, each passes its wording.
struct LoadRules {
    enum Tax { SAME, MIX, EVERY } tax = SAME;  // all files have taxids or none has | anything goes | every file must have them
    const char *no_taxid = nullptr;            // EVERY: the message, with the file name
    enum Sorted { NONE, FIRST, ALL } sorted = NONE;
    const char *unsorted = "input should be sorted: %s";
    bool sorted_before_taxid = false;          // which of the two checks speaks first about a file that fails both
    const unik::Header *against = nullptr;     // every file, the first included, is checked against this header, not the first file's
    bool announce = true;                      // the "processing file" line of --verbose
    bool concat = false;                       // the records go to Inputs::codes / taxids in file order, files[] keeps the headers
};
struct Inputs {
    vector<Loaded> files;
    int k = 0, taxid_bytes = 1;  // taxid_bytes: the widest of the files'
    bool canonical = false, hashed = false, has_taxid = false, any_taxid = false;
    unik::Header h0;
    u64 total = 0;
    // LoadRules::concat: all records in file order; a taxid per record where the inputs may carry any (MIX, unless taxids are
    // ignored) or do (the first file has them)
    vector<u64> codes;
    vector<u32> taxids;
};
static Inputs load_inputs(const vector<string> &files, const Options &o, const LoadRules &r) {
    Inputs in;
    auto check_sorted = [&](size_t i, const Loaded &L) {
        if ((r.sorted == LoadRules::ALL || (r.sorted == LoadRules::FIRST && i == 0)) && !L.h.is_sorted()) die(r.unsorted, files[i].c_str());
    };
    for (size_t i = 0; i < files.size(); i++) {
        if (r.announce) info("processing file (%zu/%zu): %s", i + 1, files.size(), files[i].c_str());
        in.files.push_back(load_unik(files[i], o));
        Loaded &L = in.files.back();
        if (i == 0) {
            in.h0 = L.h; in.k = L.h.k; in.canonical = L.h.is_canonical(); in.hashed = L.h.is_hashed();
            in.has_taxid = L.has_taxid;
        }
        if (r.against) check_compat(*r.against, L.h, files[i]);
        else if (i > 0) check_compat(in.h0, L.h, files[i]);
        if (r.sorted_before_taxid) check_sorted(i, L);
        if (r.tax == LoadRules::EVERY && !L.has_taxid) die(r.no_taxid, files[i].c_str());
        if (r.tax == LoadRules::SAME && L.has_taxid != in.has_taxid)
            die(L.has_taxid ? "taxid information not found in previous files, but found in this: %s"
                            : "taxid information found in previous files, but missing in this: %s", files[i].c_str());
        if (!r.sorted_before_taxid) check_sorted(i, L);
        in.any_taxid |= L.has_taxid;
        in.taxid_bytes = std::max(in.taxid_bytes, (int)L.h.taxid_bytes);
        in.total += L.codes.size();
        if (r.concat) {
            in.codes.insert(in.codes.end(), L.codes.begin(), L.codes.end());
            if (r.tax == LoadRules::MIX ? !o.ignore_taxid : in.has_taxid) append_taxids(L, L.taxids, 0, L.codes.size(), in.taxids);
            vector<u64>().swap(L.codes);
            vector<u32>().swap(L.taxids);
        }
    }
    return in;
}
struct Ptrs {
    vector<const u64 *> k;
    vector<const u32 *> t;
    vector<u32> ft;  // per-file taxids (ukm_*_ft): the global taxid of a file whose records carry none
    vector<u64> n;
};
static Ptrs ptrs_of(const Inputs &in, bool tax) {
    Ptrs p;
    for (auto &L : in.files) {
        p.k.push_back(L.codes.data());
        p.t.push_back(tax && L.per_record() ? L.taxids.data() : nullptr);
        p.ft.push_back(tax && L.has_taxid && !L.per_record() ? L.file_taxid : 0u);
        p.n.push_back(L.codes.size());
    }
    return p;
}
// the flags of an output that follows the header h0
static u32 out_mode(const unik::Header &h0, bool sorted, bool tax, const Options &o) {
    u32 mode = 0;
    if (sorted) mode |= unik::UnikSorted;
    else if (o.compact && !h0.is_hashed()) mode |= unik::UnikCompact;
    if (h0.is_canonical()) mode |= unik::UnikCanonical;
    if (tax) mode |= unik::UnikIncludeTaxID;
    if (h0.is_hashed()) mode |= unik::UnikHashed;
    return mode;
}

// ---- writers ----------------------------------------------------------------------------------------
// the records behind a Writer's header: encoded by ukm_unik_encode where the device codec is on, else the Writer's record loop
static void write_records(unik::Writer &w, const Options &o, const u64 *codes, const u32 *taxids, u64 n) {
    const bool tx = w.h.is_include_taxid();
    bool own = false;
    ukm_ctx *c = n ? codec_ctx(o, &own) : nullptr;
    if (c && w.h.is_compact() && !w.h.is_sorted() && (w.h.k < 1 || w.h.k > 32)) c = nullptr;
    if (c && w.device_gzip()) {
        // encoded into a device buffer and deflated there: the body never crosses to the host uncompressed
        const u64 bound = ukm_unik_encode_bound(n, w.h.k, w.h.flag, w.h.taxid_bytes);
        DevMem body(c, bound);
        u64 m = 0, nf = 0;
        const int rc = ukm_unik_encode(c, codes, tx ? taxids : nullptr, n, w.h.k, w.h.flag, w.h.taxid_bytes, (uint8_t *)body.p, bound, &m);
        if (rc == UKM_ERR_UNSORTED) throw unik::Error("codes written to a sorted .unik must be ascending");
        ck(rc);
        const u64 fbound = ukm_deflate_bound(m, 0);
        std::unique_ptr<uint8_t[]> frag(new uint8_t[fbound]);
        uint32_t crc = 0;
        ck(ukm_deflate(c, (const uint8_t *)body.p, m, 0, frag.get(), fbound, &nf, &crc));
        if (own) ck(ukm_ctx_trim(c));
        w.write_body_deflated(frag.get(), nf, crc, m);
        return;
    }
    if (c) {
        const u64 bound = ukm_unik_encode_bound(n, w.h.k, w.h.flag, w.h.taxid_bytes);
        std::unique_ptr<uint8_t[]> body(new uint8_t[bound]);  // (not a vector: nothing here needs 1.7 GB of zeros first)
        u64 m = 0;
        const int rc = ukm_unik_encode(c, codes, tx ? taxids : nullptr, n, w.h.k, w.h.flag, w.h.taxid_bytes, body.get(), bound, &m);
        if (rc == UKM_ERR_UNSORTED) throw unik::Error("codes written to a sorted .unik must be ascending");
        ck(rc);
        if (own) ck(ukm_ctx_trim(c));
        w.write_body(body.get(), m);
        return;
    }
    for (u64 i = 0; i < n; i++) {
        if (tx) w.write_code_with_taxid(codes[i], taxids[i]);
        else w.write_code(codes[i]);
    }
}
// whether an output of n records is written in device-gzip mode: asked for, compressed at a level other than 0, and there is
// a device codec to encode the body where ukm_deflate will find it
static bool device_gzip_for(const Options &o, u64 n) {
    bool own = false;
    return o.compress && o.device_gzip && o.level != 0 && n && codec_ctx(o, &own) != nullptr;
}
static void finish_unik(unik::OutStream &os, unik::Writer &w, const Options &o, const string &out_file, const u64 *codes, const u32 *taxids, u64 n) {
    w.set_number(n);
    write_records(w, o, codes, taxids, n);
    w.flush();
    os.close();
    info("%llu k-mers saved to %s", (unsigned long long)n, out_file.c_str());
}
static void write_unik(const string &out_file, const Options &o, int k, u32 mode, u32 max_taxid, u32 global_taxid,
                       const unik::Header *scale_from, const u64 *codes, const u32 *taxids, u64 n) {
    unik::OutStream os(out_file, o.compress, o.level, device_gzip_for(o, n));
    unik::Writer w(os, k, mode);
    w.set_max_taxid(max_taxid);
    if (global_taxid) w.set_global_taxid(global_taxid);
    if (scale_from && scale_from->is_scaled()) w.set_scale(scale_from->scale, scale_from->max_hash);
    finish_unik(os, w, o, out_file, codes, taxids, n);
}
// an output that follows an input header (filter.go:123-125, sample.go:116-122): no global taxid, the reader's taxid width
static void write_following(const string &out_file, const Options &o, const unik::Header &h0, u32 mode, const u64 *codes, const u32 *taxids, u64 n) {
    unik::OutStream os(out_file, o.compress, o.level, device_gzip_for(o, n));
    unik::Writer w(os, h0.k, mode & ~(u32)unik::UnikScaled);
    w.h.taxid_bytes = h0.taxid_bytes;
    if (mode & unik::UnikScaled) w.set_scale(h0.scale, h0.max_hash);
    finish_unik(os, w, o, out_file, codes, taxids, n);
}

// ---- steps on the device that several commands share ------------------------------------------------------
// codes (with their taxids, where given) sorted in place; then ukm_unique in `mode` into out / tout.  Host or device memory.
static void sort_records(Gpu &g, u64 *codes, u32 *taxids, u64 n, int key_bits) {
    if (taxids) ck(ukm_sort_pairs(g.c, codes, taxids, n, key_bits));
    else ck(ukm_sort_u64(g.c, codes, n, key_bits));
}
static u64 sort_then_unique(Gpu &g, u64 *codes, u32 *taxids, u64 n, int key_bits, int mode, u64 *out, u32 *tout, u64 cap) {
    u64 m = 0;
    if (!n) return 0;
    sort_records(g, codes, taxids, n, key_bits);
    ck(ukm_unique(g.c, codes, taxids, n, mode, out, taxids ? tout : nullptr, cap, &m));
    return m;
}
// Selection per file, the kept records in input order: `call` runs one library call over a file's records -- codes, the
// file's own taxid column or nullptr, the outputs and their capacity, the count -- and returns its status.  With `tax`
// every kept record gets its taxid: its own, or the file's.
template <class Call>
static void select_per_file(const Inputs &in, bool tax, vector<u64> &codes, vector<u32> &taxids, Call call) {
    vector<u64> ok;
    vector<u32> ot;
    for (auto &L : in.files) {
        if (L.codes.empty()) continue;
        ok.resize(L.codes.size());
        const bool own = tax && L.per_record();
        if (own) ot.resize(L.codes.size());
        u64 n = 0;
        ck(call(L, own ? L.taxids.data() : nullptr, ok.data(), own ? ot.data() : nullptr, (u64)ok.size(), &n));
        codes.insert(codes.end(), ok.begin(), ok.begin() + (long)n);
        if (tax) append_taxids(L, ot, 0, n, taxids);
    }
}
// ntHash of whole k-mers given as text (dump -H, encode -H, grep: dump.go:250-275, encode.go:106-113): every line is one
// record of k bases with exactly one window, hashed on the device in batches
static void hash_kmers_on_device(Gpu &g, const vector<string> &kmers, int k, bool canonical, vector<u64> &out) {
    out.resize(kmers.size());
    const size_t batch = 1u << 22;
    vector<uint8_t> bases;
    vector<u64> off;
    for (size_t b0 = 0; b0 < kmers.size(); b0 += batch) {
        const size_t n = std::min(batch, kmers.size() - b0);
        bases.resize(n * (size_t)k);
        off.resize(n + 1);
        for (size_t i = 0; i < n; i++) {
            memcpy(&bases[i * (size_t)k], kmers[b0 + i].data(), (size_t)k);
            off[i] = (u64)i * (u64)k;
        }
        off[n] = (u64)n * (u64)k;
        u64 m = 0;
        ck(ukm_nthash(g.c, bases.data(), off.data(), n, k, canonical ? 1 : 0, 0, 0, out.data() + b0, n, &m));
        if (m != n) die("ntHash: %llu hashes for %zu k-mers", (unsigned long long)m, n);
    }
}
