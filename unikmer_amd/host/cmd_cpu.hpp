// cmd_cpu.hpp — the commands that need no GPU: view, dump, num, info/stats, concat, head, encode, decode
// (view -g and the -H forms of dump / encode hash on the device)
// Where there is a device, dump without -H parses its text with ukm_dump and -- under UNIKMER_DEVICE_TEXT=1: a small file is
// printed sooner without a context, DESIGN.md 4.18 -- view without -g renders its text with ukm_view (records.hpp: text_ctx).
// The host loops below are what runs without a device, under UNIKMER_HOST_TEXT=1, and for dump whenever a line is outside
// ukm_dump's strict grammar: they define what both commands print, read and say.
#pragma once
#include "records.hpp"

// the format of `view`'s flags, in the precedence of the host loop: -a > -q > -t > -T > -N > -n > plain
static u32 view_format(const Args &a) {
    const u32 t = a.has("show-taxid") ? UKM_VIEW_WITH_TAXID : 0u;
    if (a.has("fasta")) return UKM_VIEW_FASTA | t;
    if (a.has("fastq")) return UKM_VIEW_FASTQ | t;
    if (a.has("show-taxid")) return UKM_VIEW_KMER_TAXID;
    if (a.has("show-taxid-only")) return UKM_VIEW_TAXID;
    if (a.has("show-code-only")) return UKM_VIEW_CODE;
    if (a.has("show-code")) return UKM_VIEW_KMER_CODE;
    return UKM_VIEW_KMER;
}
// One file through ukm_view, in chunks of records that bound the text buffer.  What is printed as a record's taxid is what
// unik::Reader::read hands out: its own, else the header's global taxid -- also under -I, which the loader is not told about.
static void view_on_device(ukm_ctx *c, bool own, const string &file, const Options &o, u32 fmt, unik::OutStream &out) {
    Options ol = o;
    ol.ignore_taxid = false;
    const Loaded L = load_unik(file, ol);
    const int k = L.h.k, hashed = L.h.is_hashed() ? 1 : 0;
    const u64 n = L.codes.size(), chunk = std::max<u64>(1, (256ull << 20) / ukm_view_bound(1, k, hashed, fmt));
    if (!n) return;
    const u64 cap = ukm_view_bound(std::min(n, chunk), k, hashed, fmt);
    std::unique_ptr<uint8_t[]> text(new uint8_t[cap]);
    for (u64 i = 0; i < n; i += chunk) {
        const u64 m = std::min(chunk, n - i);
        u64 bytes = 0;
        ck(ukm_view(c, L.codes.data() + i, L.h.is_include_taxid() ? L.taxids.data() + i : nullptr, L.h.global_taxid, m, k, hashed, fmt,
                    text.get(), cap, &bytes));
        out.write(text.get(), bytes);
    }
    if (own) ck(ukm_ctx_trim(c));
}

static int cmd_view(int argc, char **argv) {  // view.go:163-218
    Args a = parse_args(argc, argv, {{'o', "out-file", true}, {'n', "show-code", false}, {'N', "show-code-only", false}, {'a', "fasta", false},
                                     {'q', "fastq", false}, {'t', "show-taxid", false}, {'T', "show-taxid-only", false}, {'g', "genome", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    vector<string> genomes;
    if (a.has("genome")) {  // comma-separated list (a StringSlice flag in view.go:235)
        std::istringstream gs(a.str("genome", ""));
        string gfile;
        while (std::getline(gs, gfile, ',')) if (!gfile.empty()) genomes.push_back(gfile);
    }
    auto out = text_out(a.str("out-file", "-"));
    string buf;
    // -g: hash -> first location in the genomes (loadHash2Loc, util.go:344-393: canonical ntHash of every window of
    // every CIRCULAR record, the first occurrence wins).  On the device: ukm_nthash of all records, a stable sort of
    // (hash, window index), one lower bound per queried code.
    SeqBatch gb;
    vector<u64> gh, gwoff;  // sorted hashes; first window index of every record
    vector<u32> gpos;       // window index of gh[i]
    std::unique_ptr<Gpu> gpu;
    bool g_loaded = false;
    auto load_genomes = [&](int k) {
        for (auto &gf : genomes) read_fastx(gf, gb, false);
        const u64 nrec = gb.off.size() - 1;
        gwoff.assign(nrec + 1, 0);
        for (u64 r = 0; r < nrec; r++) { const u64 len = gb.off[r + 1] - gb.off[r]; gwoff[r + 1] = gwoff[r] + (len >= (u64)k ? len : 0); }
        const u64 nw = gwoff[nrec];
        if (nw > 0xFFFFFFFFull) die("-g/--genome: more than 2^32 k-mers in the genomes");
        gh.resize(nw); gpos.resize(nw);
        if (nw == 0) return;
        gpu.reset(new Gpu(o.gpu));
        u64 m = 0;
        ck(ukm_nthash(gpu->c, gb.bases.data(), gb.off.data(), nrec, k, 1, 1, 0, gh.data(), nw, &m));
        if (m != nw) die("-g/--genome: %llu hashes for %llu windows", (unsigned long long)m, (unsigned long long)nw);
        for (u64 i = 0; i < nw; i++) gpos[i] = (u32)i;
        ck(ukm_sort_pairs(gpu->c, gh.data(), gpos.data(), nw, 64));
        info("%llu hash-k-mers pairs from %llu sequences loaded", (unsigned long long)nw, (unsigned long long)nrec);
    };
    bool text_own = false;
    ukm_ctx *text_c = genomes.empty() ? text_ctx(o, o.device_view, &text_own) : nullptr;  // (with -g the host loop, also where -g is ignored)
    for (auto &f : files) {
        if (text_c) { view_on_device(text_c, text_own, f, o, view_format(a), *out); continue; }
        unik::Reader r(f);
        const int k = r.h.k;
        const bool hashed = r.h.is_hashed();
        const string qual((size_t)k, 'g');
        bool use_genomes = false;
        if (!genomes.empty()) {
            if (!hashed) warn("-g/--genome ignored since k-mers not hashed");
            else if (!r.h.is_canonical()) warn("-g/--genome ignored since 'canonical' flag is off");
            else { if (!g_loaded) { load_genomes(k); g_loaded = true; } use_genomes = true; }
        }
        vector<u64> qcodes;
        vector<u32> qtax;
        vector<string> qkmer;
        if (use_genomes) {  // all codes of the file first, then one batch of lower bounds on the device
            u64 c; u32 t;
            while (r.read(c, t)) { qcodes.push_back(c); qtax.push_back(t); }
            qkmer.resize(qcodes.size());
            vector<u64> cuts;
            const size_t batch = 1u << 28;
            for (size_t b0 = 0; b0 < qcodes.size(); b0 += batch) {
                const size_t nq = std::min(batch, qcodes.size() - b0);
                cuts.resize(nq);
                if (!gh.empty()) ck(ukm_partition_points(gpu->c, gh.data(), gh.size(), qcodes.data() + b0, (int)nq, cuts.data()));
                for (size_t i = 0; i < nq; i++) {
                    const u64 code = qcodes[b0 + i];
                    const u64 lb = gh.empty() ? 0 : cuts[i];
                    if (lb < gh.size() && gh[lb] == code) {
                        const u64 w = gpos[lb];
                        const u64 rec = (u64)(std::upper_bound(gwoff.begin(), gwoff.end(), w) - gwoff.begin()) - 1;
                        const u64 len = gb.off[rec + 1] - gb.off[rec], idx = w - gwoff[rec];
                        string km((size_t)k, 'N');
                        for (int j = 0; j < k; j++) km[(size_t)j] = (char)gb.bases[gb.off[rec] + (idx + (u64)j) % len];
                        qkmer[b0 + i] = km;
                    } else {
                        qkmer[b0 + i] = std::to_string(code);
                        warn("fail to decode hash: %llu, which is not found in given genomes", (unsigned long long)code);
                    }
                }
            }
        }
        u64 code; u32 taxid;
        size_t qi = 0;
        for (;;) {
            if (use_genomes) { if (qi >= qcodes.size()) break; code = qcodes[qi]; taxid = qtax[qi]; }
            else if (!r.read(code, taxid)) break;
            const string kmer = use_genomes ? qkmer[qi++] : (hashed ? std::to_string(code) : decode_kmer(code, k));
            if (a.has("fasta")) buf += ">" + std::to_string(code) + (a.has("show-taxid") ? " " + std::to_string(taxid) : "") + "\n" + kmer + "\n";
            else if (a.has("fastq")) buf += "@" + std::to_string(code) + (a.has("show-taxid") ? " " + std::to_string(taxid) : "") + "\n" + kmer + "\n+\n" + qual + "\n";
            else if (a.has("show-taxid")) buf += kmer + "\t" + std::to_string(taxid) + "\n";
            else if (a.has("show-taxid-only")) buf += std::to_string(taxid) + "\n";
            else if (a.has("show-code-only")) buf += std::to_string(code) + "\n";
            else if (a.has("show-code")) buf += kmer + "\t" + std::to_string(code) + "\n";
            else buf += kmer + "\n";
            if (buf.size() > (1u << 20)) { put(*out, buf); buf.clear(); }
        }
    }
    put(*out, buf);
    return 0;
}

// The texts of `dump` through ukm_dump: false when a line is outside its grammar (or there is nothing it could be asked: no
// line, a k it does not take) -- nothing has been written then, and the host loop runs over the same texts.  k and whether
// there are two columns come from the first non-empty line, as in the host loop; -u is applied here, first occurrences kept.
static bool dump_on_device(ukm_ctx *c, bool own, const vector<string> &texts, bool decimal, bool canonical, bool canonical_only, bool unique,
                           int &k, bool &include_taxid, vector<u64> &codes, vector<u32> &taxids) {
    bool found = false;
    for (auto &t : texts) {
        std::istringstream ss(t);
        string line;
        while (!found && std::getline(ss, line)) {
            trim_line_end(line);
            if (line.empty()) continue;
            const size_t tab = line.find_first_of("\t ");
            if (!decimal) k = (int)(tab == string::npos ? line.size() : tab);
            include_taxid = tab != string::npos;
            found = true;
        }
        if (found) break;
    }
    if (!found || k < 1 || k > (decimal ? 64 : 32)) return false;
    const u32 flags = (include_taxid ? UKM_DUMP_TAXID : 0u) | (decimal ? UKM_DUMP_DECIMAL : 0u) |
                      (!decimal && canonical ? UKM_DUMP_CANONICAL : 0u) | (!decimal && canonical_only ? UKM_DUMP_CANONICAL_ONLY : 0u);
    u64 n = 0;
    for (auto &t : texts) {
        const u64 cap = (u64)std::count(t.begin(), t.end(), '\n') + 1;
        codes.resize(n + cap);
        if (include_taxid) taxids.resize(n + cap);
        u64 m = 0;
        const int rc = ukm_dump(c, (const uint8_t *)t.data(), t.size(), k, flags, codes.data() + n, include_taxid ? taxids.data() + n : nullptr,
                                cap, &m, nullptr);
        if (rc == UKM_ERR_FORMAT) return false;
        ck(rc);
        n += m;
    }
    if (own) ck(ukm_ctx_trim(c));
    if (unique) {
        std::set<u64> seen;
        u64 kept = 0;
        for (u64 i = 0; i < n; i++) {
            if (!seen.insert(codes[i]).second) continue;
            codes[kept] = codes[i];
            if (include_taxid) taxids[kept] = taxids[i];
            kept++;
        }
        n = kept;
    }
    codes.resize(n);
    if (include_taxid) taxids.resize(n);
    return true;
}

static int cmd_dump(int argc, char **argv) {  // dump.go:128-315
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'u', "unique", false}, {'K', "canonical", false}, {'O', "canonical-only", false},
                                     {'s', "sorted", false}, {'t', "taxid", true}, {'H', "hash", false}, {0, "hashed", false}, {'k', "kmer-len", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const bool hashed = a.has("hash");  // compute the ntHash of the given k-mers (dump.go:73)
    if (hashed && a.has("canonical-only")) die("flag -H/--hash and -k/--canonical-only are not compatible");  // dump.go:76-78
    const bool hashed_already = a.has("hashed");
    bool canonical = a.has("canonical");
    const bool canonical_only = a.has("canonical-only"), sorted = a.has("sorted"), unique = a.has("unique");
    int k = -1;
    if (hashed_already) { canonical = true; k = (int)a.num("kmer-len", 0); if (k == 0) die("flag -k/--kmer-len should be given when --hashed given"); }
    const u32 gtaxid = (u32)a.num("taxid", 0);
    const string out_file = out_name(a.str("out-prefix", "-"));
    unik::OutStream os(out_file, o.compress, o.level);
    std::unique_ptr<unik::Writer> w;
    std::set<u64> seen;
    u64 n = 0;
    bool include_taxid = false;
    vector<string> hk;  // -H: the k-mers of all files, hashed on the device after the last line
    vector<u32> ht;
    // the first line fixes k and whether taxids are included (dump.go:139-223)
    auto open_writer = [&]() {
        u32 mode = 0;
        if (sorted) mode |= unik::UnikSorted;
        else if (o.compact && !hashed_already && !hashed) mode |= unik::UnikCompact;
        if (canonical || canonical_only) mode |= unik::UnikCanonical;
        if (include_taxid) mode |= unik::UnikIncludeTaxID;
        if (hashed_already || hashed) mode |= unik::UnikHashed;
        w.reset(new unik::Writer(os, k, mode));
        w->set_max_taxid(o.max_taxid);
        if (gtaxid && !include_taxid) w->set_global_taxid(gtaxid);
    };
    vector<string> texts;  // read once: the device path and the host loop behind it see the same bytes (a file may be stdin)
    for (auto &f : files) texts.push_back(read_text(f));
    bool text_own = false;
    ukm_ctx *text_c = hashed ? nullptr : text_ctx(o, o.device_dump, &text_own);
    if (text_c) {
        vector<u64> dc;
        vector<u32> dt;
        int dk = k;
        bool dtax = false;
        if (dump_on_device(text_c, text_own, texts, hashed_already, canonical, canonical_only, unique, dk, dtax, dc, dt)) {
            k = dk;
            include_taxid = dtax;
            open_writer();
            write_records(*w, o, dc.data(), dt.data(), dc.size());
            n = dc.size();
            texts.clear();
        }
    }
    for (auto &text : texts) {
        std::istringstream ss(text);
        string line;
        while (std::getline(ss, line)) {
            trim_line_end(line);
            if (line.empty()) continue;
            u32 taxid = 0;
            string kmer = line;
            size_t tab = line.find_first_of("\t ");
            bool has_t = false;
            if (tab != string::npos) { kmer = line.substr(0, tab); taxid = (u32)strtoul(line.c_str() + tab + 1, nullptr, 10); has_t = true; }
            if (!w) {
                if (!hashed_already) k = (int)kmer.size();
                if (k > 32 && !hashed_already && !hashed) die("k-mer size (%d) should be <= 32", k);
                if (k > 64) die("k-mer size (%d) should be <= 64", k);
                include_taxid = has_t;
                open_writer();
            }
            u64 code;
            if (hashed) {
                if ((int)kmer.size() != k) die("K-mer length mismatch, previous: %d, current: %zu. %s", k, kmer.size(), kmer.c_str());
                hk.push_back(kmer);
                ht.push_back(taxid);
                continue;
            }
            if (hashed_already) code = strtoull(kmer.c_str(), nullptr, 10);
            else {
                if ((int)kmer.size() != k) die("K-mer length mismatch, previous: %d, current: %zu. %s", k, kmer.size(), kmer.c_str());
                if (!encode_kmer(kmer, code)) die("fail to encode '%s': illegal base", kmer.c_str());
                const u64 rc = revcomp(code, k);
                if (canonical_only) { if (rc < code) continue; }
                else if (canonical && rc < code) code = rc;
            }
            if (unique && !seen.insert(code).second) continue;
            if (include_taxid) w->write_code_with_taxid(code, taxid); else w->write_code(code);
            n++;
        }
    }
    if (!w) die("no k-mers given");
    if (hashed) {
        Gpu g(o.gpu);
        vector<u64> hv;
        hash_kmers_on_device(g, hk, k, canonical, hv);
        for (size_t i = 0; i < hv.size(); i++) {
            if (unique && !seen.insert(hv[i]).second) continue;
            if (include_taxid) w->write_code_with_taxid(hv[i], ht[i]); else w->write_code(hv[i]);
            n++;
        }
    }
    w->flush();
    os.close();
    info("%llu unique k-mers saved to %s", (unsigned long long)n, out_file.c_str());
    return 0;
}

static int cmd_num(int argc, char **argv) {  // num.go:60-131
    Args a = parse_args(argc, argv, {{'o', "out-file", true}, {'n', "file-name", false}, {'b', "basename", false}, {'f', "force", false}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    auto out = text_out(a.str("out-file", "-"));
    for (auto &f : files) {
        unik::Reader r(f);
        long long n = (r.h.number == ~0ull || r.h.number == 0) ? -1 : (long long)r.h.number;
        if (n < 0 && a.has("force")) { u64 c; u32 t; n = 0; while (r.read(c, t)) n++; }
        string line = std::to_string(n);
        if (a.has("file-name")) line += "\t" + (a.has("basename") ? base_of(f) : f);
        put(*out, line + "\n");
    }
    return 0;
}

static int cmd_info(int argc, char **argv) {  // info.go:377-421 (tabular form)
    Args a = parse_args(argc, argv, {{'o', "out-file", true}, {'a', "all", false}, {'T', "tabular", false}, {'e', "skip-err", false},
                                     {0, "symbol-true", true}, {0, "symbol-false", true}, {'b', "basename", false}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    auto out = text_out(a.str("out-file", "-"));
    const string T = a.str("symbol-true", "✓"), F = a.str("symbol-false", "✕");
    string hdr = "file\tk\tcanonical\thashed\tscaled\tinclude-taxid\tglobal-taxid\tsorted";
    if (a.has("all")) hdr += "\tcompact\tgzipped\tversion\tnumber\tdescription";
    put(*out, hdr + "\n");
    for (auto &f : files) {
        unik::Reader r(f);
        auto b = [&](bool v) { return v ? T : F; };
        string line = (a.has("basename") ? base_of(f) : f) + "\t" + std::to_string(r.h.k) + "\t" + b(r.h.is_canonical()) + "\t" + b(r.h.is_hashed()) +
                      "\t" + b(r.h.is_scaled()) + "\t" + b(r.h.is_include_taxid()) + "\t" + (r.h.has_global_taxid() ? std::to_string(r.h.global_taxid) : "") +
                      "\t" + b(r.h.is_sorted());
        if (a.has("all")) {
            long long n = (r.h.number == ~0ull || r.h.number == 0) ? -1 : (long long)r.h.number;
            if (n < 0) { u64 c; u32 t; n = 0; while (r.read(c, t)) n++; }
            line += "\t" + b(r.h.is_compact()) + "\t" + b(r.gzipped()) + "\tv" + std::to_string(r.h.main_version) + "." + std::to_string(r.h.minor_version) +
                    "\t" + std::to_string(n) + "\t" + r.h.description;
        }
        put(*out, line + "\n");
    }
    return 0;
}

static int cmd_concat(int argc, char **argv) {  // concat.go:60-206
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'s', "sorted", false}, {'t', "taxid", true}, {'n', "number", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const string out_file = out_name(a.str("out-prefix", "-"));
    unik::OutStream os(out_file, o.compress, o.level);
    std::unique_ptr<unik::Writer> w;
    unik::Header h0;
    bool tax = false;
    u64 n = 0;
    for (size_t i = 0; i < files.size(); i++) {
        unik::Reader r(files[i]);
        if (!w) {
            h0 = r.h;
            tax = !o.ignore_taxid && r.h.has_taxid_info();
            w.reset(new unik::Writer(os, r.h.k, out_mode(r.h, a.has("sorted"), tax, o)));
            w->set_max_taxid(o.max_taxid);
            if (r.h.is_scaled()) w->set_scale(r.h.scale, r.h.max_hash);
            const long long num = a.num("number", -1);
            w->set_number(num < 0 ? ~0ull : (u64)num);  // concat.go:69,143-145: unknown unless given
        } else {
            check_compat(h0, r.h, files[i]);
        }
        u64 c; u32 t;
        while (r.read(c, t)) { if (tax) w->write_code_with_taxid(c, t); else w->write_code(c); n++; }
    }
    if (!w) die("no input");
    w->flush();
    os.close();
    info("%llu k-mers saved to %s", (unsigned long long)n, out_file.c_str());
    return 0;
}

static int cmd_head(int argc, char **argv) {  // head.go:60-163
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'n', "number", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    if (files.size() > 1) die("no more than one file should be given");
    const long long number = a.num("number", 10);
    if (number <= 0) die("value of flag -n/--number should be positive");
    unik::Reader r(files[0]);
    const string out_file = out_name(a.str("out-prefix", "-"));
    unik::OutStream os(out_file, o.compress, o.level);
    unik::Header h = r.h;
    unik::Writer w(os, h.k, h.flag & ~(u32)unik::UnikScaled);
    w.h.taxid_bytes = h.taxid_bytes; w.h.global_taxid = h.global_taxid; w.h.description = h.description;
    if (h.is_scaled()) w.set_scale(h.scale, h.max_hash);
    u64 c; u32 t; long long n = 0;
    vector<std::pair<u64, u32>> recs;
    while (n < number && r.read(c, t)) { recs.push_back({c, t}); n++; }
    w.set_number((u64)n);
    for (auto &x : recs) { if (h.is_include_taxid()) w.write_code_with_taxid(x.first, x.second); else w.write_code(x.first); }
    w.flush();
    os.close();
    return 0;
}

static int cmd_encode(int argc, char **argv) {  // encode.go:60-136
    Args a = parse_args(argc, argv, {{'o', "out-file", true}, {'a', "all", false}, {'K', "canonical", false}, {'H', "hash", false}});
    Options o = get_options(a);
    const bool hashed = a.has("hash");
    vector<string> files = get_files(a, o);
    auto out = text_out(a.str("out-file", "-"));
    vector<string> kmers;  // -H (encode.go:106-113): one ntHash per line, the first line fixes k (<= 64)
    int hk = -1;
    for (auto &f : files) {
        std::istringstream ss(read_text(f));
        string line;
        while (std::getline(ss, line)) {
            trim_line_end(line);
            if (line.empty()) continue;
            if (hashed) {
                if (hk == -1) { hk = (int)line.size(); if (hk > 64) die("k-mer size (%d) should be <=64", hk); }
                else if ((int)line.size() != hk) die("K-mer length mismatch, previous: %d, current: %zu. %s", hk, line.size(), line.c_str());
                kmers.push_back(line);
                continue;
            }
            u64 code;
            if (!encode_kmer(line, code)) die("fail to encode '%s'", line.c_str());
            const int k = (int)line.size();
            if (a.has("canonical")) code = std::min(code, revcomp(code, k));
            if (a.has("all")) put(*out, line + "\t" + decode_kmer(code, k) + "\t" + std::to_string(code) + "\n");
            else put(*out, std::to_string(code) + "\n");
        }
    }
    if (kmers.empty()) return 0;
    Gpu g(o.gpu);
    vector<u64> hv;
    hash_kmers_on_device(g, kmers, hk, a.has("canonical"), hv);
    string buf;
    for (u64 h : hv) { buf += std::to_string(h) + "\n"; if (buf.size() > (1u << 20)) { put(*out, buf); buf.clear(); } }
    put(*out, buf);
    return 0;
}

static int cmd_decode(int argc, char **argv) {  // decode.go:60-124
    Args a = parse_args(argc, argv, {{'o', "out-file", true}, {'k', "kmer-len", true}, {'a', "all", false}});
    Options o = get_options(a);
    const int k = (int)a.num("kmer-len", 0);
    if (k <= 0 || k > 32) die("invalid k: %d", k);
    vector<string> files = get_files(a, o);
    auto out = text_out(a.str("out-file", "-"));
    const u64 maxcode = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    for (auto &f : files) {
        std::istringstream ss(read_text(f));
        string line;
        while (std::getline(ss, line)) {
            if (line.empty()) continue;
            const u64 code = strtoull(line.c_str(), nullptr, 10);
            if (code > maxcode) die("encode integer overflows for k=%d, max: %llu", k, (unsigned long long)maxcode);  // decode.go:102-104
            if (a.has("all")) put(*out, std::to_string(code) + "\t" + decode_kmer(code, k) + "\n");
            else put(*out, decode_kmer(code, k) + "\n");
        }
    }
    return 0;
}
