// cmd_select.hpp — record selection: sample / filter / grep (ukm_sample / ukm_filter / ukm_grep keep input order and every
// record's own taxid) and the TaxId workflow's last two steps, rfilter / tsplit
#pragma once
#include "records.hpp"

static int cmd_sample(int argc, char **argv) {  // sample.go:45-166
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'s', "start", true}, {'w', "window", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const long long start = a.num("start", 1), window = a.num("window", 1);
    if (start <= 0) die("value of flag --start should be greater than 0");
    if (window <= 0) die("value of flag --window should be greater than 0");
    const string out_file = out_name(a.str("out-prefix", "-"));
    // The header follows the first input (sample.go:116-120) and every record is written with the taxid the reader hands
    // out (:136,147), also under -I: -I only switches off the include-taxid flag for files with ONE taxid and the check that
    // all inputs agree (:114,125).  So the taxid columns are always loaded.
    Options oo = o;
    oo.ignore_taxid = false;
    LoadRules rules;
    rules.tax = o.ignore_taxid ? LoadRules::MIX : LoadRules::SAME;
    Inputs in = load_inputs(files, oo, rules);
    u32 mode = in.h0.flag;
    if (!o.ignore_taxid && in.has_taxid) mode |= unik::UnikIncludeTaxID;  // "for multiple input files"
    const bool tax = (mode & unik::UnikIncludeTaxID) != 0;
    vector<u64> codes;
    vector<u32> taxids;
    if (in.total) {
        Gpu g(o.gpu);
        select_per_file(in, tax, codes, taxids, [&](const Loaded &L, const u32 *own, u64 *ok, u32 *ot, u64 cap, u64 *n) {  // j restarts for every file (sample.go:134)
            return ukm_sample(g.c, L.codes.data(), own, L.codes.size(), (u64)start, (u64)window, ok, ot, cap, n);
        });
    }
    write_following(out_file, o, in.h0, mode, codes.data(), taxids.data(), codes.size());
    return 0;
}

static int cmd_filter(int argc, char **argv) {  // filter.go:43-168
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'v', "invert", false}, {'t', "threshold", true}, {'w', "window", true},
                                     {'s', "penalty-s", true}, {'d', "penalty-d", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    if (files.size() > 1) die("no more than one file should be given");
    const long long threshold = a.num("threshold", 15);
    if (threshold < 0) die("value of flag --threshold should be greater than or equal to 0");
    long long window = a.num("window", 7);
    if (window <= 0) die("value of flag --window should be greater than 0");
    const int ps = (int)a.num("penalty-s", 3), pd = (int)a.num("penalty-d", 1);
    const string out_file = out_name(a.str("out-prefix", "-"));
    Options oo = o;
    oo.ignore_taxid = false;  // the header follows the input (filter.go:123): records keep their taxids
    LoadRules rules;
    rules.announce = false;
    Inputs in = load_inputs(files, oo, rules);
    const int k = in.k;
    if (window > k) {
        warn("window size (%lld) is bigger than k (%d)", window, k);
        window = k;
    }
    vector<u64> codes;
    vector<u32> taxids;
    if (in.total) {
        Gpu g(o.gpu);
        select_per_file(in, in.files[0].per_record(), codes, taxids, [&](const Loaded &L, const u32 *own, u64 *ok, u32 *ot, u64 cap, u64 *n) {
            return ukm_filter(g.c, L.codes.data(), own, L.codes.size(), k, (int)window, ps, pd, (int)threshold, a.has("invert") ? UKM_F_INVERT : 0, ok, ot, cap, n);
        });
    }
    write_following(out_file, o, in.h0, in.h0.flag, codes.data(), taxids.data(), codes.size());
    return 0;
}

// =================================================================================================
// rfilter / tsplit
// =================================================================================================
// nodes.dmp with its third column: the rank of every node, lower-cased (taxdump keeps them as they are; every use in
// rfilter.go lower-cases first)
struct TaxDump {
    vector<u32> child, parent, mo, mn;
    vector<string> rank;  // of child[i]; empty when the line has no third column
};
static TaxDump read_taxdump_with_ranks(const Options &o) {
    const string nodes = o.data_dir + "/nodes.dmp", merged = o.data_dir + "/merged.dmp";
    if (!file_exists(nodes)) die("taxonomy file not found: %s (set --data-dir or UNIKMER_DB)", nodes.c_str());
    info("loading Taxonomy from: %s", o.data_dir.c_str());
    TaxDump d;
    std::ifstream fh(nodes);
    string line;
    u32 a, b;
    while (std::getline(fh, line)) {
        if (!parse_two_ids(line, a, b)) continue;
        d.child.push_back(a); d.parent.push_back(b);
        string r;
        size_t p1 = line.find('|'), p2 = p1 == string::npos ? p1 : line.find('|', p1 + 1);
        if (p2 != string::npos) {
            size_t p3 = line.find('|', p2 + 1);
            r = lower_trim(line.substr(p2 + 1, p3 == string::npos ? string::npos : p3 - p2 - 1));
        }
        d.rank.push_back(r);
    }
    if (file_exists(merged)) {
        std::ifstream mh(merged);
        while (std::getline(mh, line)) if (parse_two_ids(line, a, b)) { d.mo.push_back(a); d.mn.push_back(b); }
    }
    info("%zu nodes loaded, %zu merged nodes loaded", d.child.size(), d.mo.size());
    return d;
}
// the with-ranks variant of load_taxonomy: rank_ids numbers the rank strings 1..255
static void upload_taxonomy_with_ranks(Gpu &g, const TaxDump &d, const std::map<string, int> &rank_ids) {
    ck(ukm_taxonomy_load(g.c, d.child.data(), d.parent.data(), d.child.size(), d.mo.empty() ? nullptr : d.mo.data(),
                         d.mn.empty() ? nullptr : d.mn.data(), d.mo.size()));
    vector<uint8_t> ids(d.child.size(), 0);
    for (size_t i = 0; i < ids.size(); i++)
        if (!d.rank[i].empty()) ids[i] = (uint8_t)rank_ids.at(d.rank[i]);
    ck(ukm_taxonomy_set_ranks(g.c, d.child.data(), ids.data(), ids.size()));
}
static RankOrder read_rank_order(const Options &o, const string &rank_file) {  // rfilter.go:582-609
    if (!rank_file.empty()) {
        info("read rank order from: %s", rank_file.c_str());
        return read_rank_order_file(rank_file);
    }
    // (the reference writes its built-in list to <data-dir>/ranks.txt when that file is missing; this driver carries no list)
    const string def = o.data_dir + "/ranks.txt";
    if (!file_exists(def))
        die("default rank file not found: %s; give the ordered ranks with -r/--rank-file (type \"unikmer rfilter --help\" for the format)", def.c_str());
    info("read rank order from: %s", def.c_str());
    return read_rank_order_file(def);
}
// names by order, descending; the names of one order alphabetically
static vector<std::pair<int, string>> by_order_desc(const std::map<string, int> &m) {
    vector<std::pair<int, string>> v;
    for (auto &kv : m) v.emplace_back(kv.second, kv.first);
    std::sort(v.begin(), v.end(), [](const std::pair<int, string> &x, const std::pair<int, string> &y) {
        return x.first != y.first ? x.first > y.first : x.second < y.second;
    });
    return v;
}

static int cmd_rfilter(int argc, char **argv) {  // rfilter.go:66-341
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'r', "rank-file", true}, {0, "list-order", false}, {0, "list-ranks", false},
                                     {'N', "discard-noranks", false}, {'n', "save-predictable-norank", false}, {'B', "black-list", true},
                                     {'R', "discard-root", false}, {0, "root-taxid", true}, {'L', "lower-than", true}, {'H', "higher-than", true},
                                     {'E', "equal-to", true}});
    if (a.has("help")) {
        fprintf(stderr,
                "unikmer rfilter: filter k-mers by taxonomic rank\n\n"
                "  -o out prefix  -r rank file  --list-order  --list-ranks  -N discard ranks without order  -n keep predictable ones (with -L)\n"
                "  -B black list of ranks  -R discard the root taxid (--root-taxid, default 1)  -L / -H / -E rank limits\n\n"
                "Rank file: blank lines and lines starting with \"#\" are ignored; ranks in descending order, case ignored; ranks of the\n"
                "same order in one line separated with commas; ranks without order carry the prefix \"!\".  Without -r the file\n"
                "<data-dir>/ranks.txt is read.\n");
        return 0;
    }
    Options o = get_options(a);
    const bool list_order = a.has("list-order"), list_ranks = a.has("list-ranks");
    vector<string> files;
    if (!list_order && !list_ranks) files = get_files(a, o);
    const string lower = lower_trim(a.str("lower-than")), higher = lower_trim(a.str("higher-than"));
    vector<string> equals, black;
    for (auto &e : a.list("equal-to")) equals.push_back(lower_trim(e));
    for (auto &e : a.list("black-list")) if (!lower_trim(e).empty()) black.push_back(lower_trim(e));
    bool discard_norank = a.has("discard-noranks");
    const bool save_norank = a.has("save-predictable-norank"), discard_root = a.has("discard-root");
    if (!higher.empty() && !lower.empty()) die("-H/--higher-than and -L/--lower-than can't be simultaneous given");
    if (save_norank) {
        discard_norank = true;
        if (lower.empty()) die("flag -n/--save-predictable-norank only works along with -L/--lower-than");
    }
    RankOrder ro = read_rank_order(o, a.str("rank-file"));
    if (list_order) {  // needs no taxonomy and no device
        int pre = -1;
        for (auto &p : by_order_desc(ro.order)) {
            if (p.first == pre) printf(",%s", p.second.c_str());
            else { if (pre != -1) printf("\n"); printf("%s", p.second.c_str()); pre = p.first; }
        }
        printf("\n");
        return 0;
    }
    TaxDump dump = read_taxdump_with_ranks(o);
    std::map<string, int> rank_ids;  // the taxonomy's rank strings, numbered 1.. in sorted order
    for (auto &r : dump.rank) if (!r.empty()) rank_ids[r] = 0;
    {
        vector<string> undefined;
        int id = 0;
        for (auto &kv : rank_ids) {
            kv.second = ++id;
            if (!ro.order.count(kv.first) && !ro.noranks.count(kv.first)) undefined.push_back(kv.first);
        }
        if (!undefined.empty()) {
            string joined;
            for (auto &r : undefined) joined += (joined.empty() ? "" : ", ") + r;
            die("rank order not defined in rank file: %s", joined.c_str());
        }
        if (id > 255) die("%d different ranks in %s/nodes.dmp; rank ids are one byte (at most 255)", id, o.data_dir.c_str());
    }
    if (list_ranks) {
        std::map<string, int> m;
        for (auto &kv : rank_ids) m[kv.first] = ro.order.count(kv.first) ? ro.order[kv.first] : 0;
        for (auto &p : by_order_desc(m)) printf("%s\n", p.second.c_str());
        return 0;
    }
    // newRankFilter (rfilter.go:371-436) in rank ids
    ukm_rank_filter f;
    memset(&f, 0, sizeof(f));
    auto order_of = [&](const string &rank) -> int {  // getRankOrder
        if (!ro.order.count(rank)) die("rank order not defined in rank file: %s", rank.c_str());
        if (!rank_ids.count(rank)) die("rank order not found in taxonomy database: %s", rank.c_str());
        return ro.order[rank];
    };
    for (auto &kv : rank_ids) {
        if (ro.order.count(kv.first)) f.order[kv.second] = ro.order[kv.first];
        if (ro.noranks.count(kv.first)) f.no_rank[kv.second] = 1;
    }
    for (auto &r : black) if (rank_ids.count(r)) f.black[rank_ids[r]] = 1;
    if (!lower.empty()) f.lower = order_of(lower);
    if (!higher.empty()) f.higher = order_of(higher);
    {
        std::set<int> oe;
        for (auto &e : equals) oe.insert(order_of(e));
        if (oe.size() > 32) die("more than 32 different rank orders given with -E/--equal-to");
        for (int v : oe) f.equal[f.n_equal++] = v;
    }
    f.discard_norank = discard_norank; f.save_norank = save_norank; f.discard_root = discard_root;
    f.root_taxid = (u32)a.num("root-taxid", 1);
    // the inputs, all of them before a device is touched: every file needs taxid information (rfilter.go:260-278)
    const string out_file = out_name(a.str("out-prefix", "-"));
    LoadRules rules;
    rules.tax = LoadRules::EVERY;
    rules.no_taxid = "taxid information not found: %s";
    Inputs in = load_inputs(files, o, rules);
    vector<u64> codes;
    vector<u32> taxids;
    if (in.total) {
        Gpu g(o.gpu);
        upload_taxonomy_with_ranks(g, dump, rank_ids);
        select_per_file(in, true, codes, taxids, [&](const Loaded &L, const u32 *own, u64 *ok, u32 *ot, u64 cap, u64 *n) {
            return ukm_rfilter(g.c, L.codes.data(), own, L.file_taxid, L.codes.size(), &f, ok, ot, cap, n);
        });
    }
    // the output flag: the first input's | include-taxid; the taxid width follows that reader (rfilter.go:268-272)
    write_following(out_file, o, in.h0, in.h0.flag | unik::UnikIncludeTaxID, codes.data(), taxids.data(), codes.size());
    return 0;
}

static int cmd_tsplit(int argc, char **argv) {  // tsplit.go:58-300
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'O', "out-dir", true}, {0, "force", false}});
    Options o = get_options(a);
    const string prefix = a.has("out-prefix") ? a.str("out-prefix") : string("tsplit");
    if (prefix.empty() || prefix[0] == '.') die("-o/--out-prefix should not be empty or starting with \".\"");
    vector<string> files = get_files(a, o);
    string outdir = a.str("out-dir");
    if (outdir.empty()) outdir = files[0] == "-" ? "stdin.tsplit" : files[0] + ".tsplit";
    // the inputs (all of them before the directory and the device are touched): records are read with the taxid the
    // reader hands out -- their own, the file's global one, or 0 -- also under -I, which only switches off the check that
    // the files agree (tsplit.go:149,163,176)
    Options oo = o;
    oo.ignore_taxid = false;
    LoadRules rules;
    rules.tax = o.ignore_taxid ? LoadRules::MIX : LoadRules::SAME;
    rules.sorted = LoadRules::FIRST;
    rules.concat = true;
    Inputs in = load_inputs(files, oo, rules);
    const unik::Header &h0 = in.h0;
    const u64 n = in.total;
    in.taxids.resize(n);  // (files that agree on carrying no taxid information: every record has taxid 0)
    {   // tsplit.go:92-110: an output directory that is not empty is emptied with --force, and only warned about without
        char cwd[4096];
        const string pwd = getcwd(cwd, sizeof cwd) ? cwd : "";
        if (outdir != "./" && outdir != "." && outdir != pwd) {
            if (dir_exists(outdir)) {
                vector<string> names = list_dir(outdir);
                if (a.has("force")) empty_dir(outdir, names);
                else if (!names.empty()) warn("outdir not empty: %s, you can use --force to overwrite", outdir.c_str());
            } else {
                prepare_dir(outdir, false, "out-dir");
            }
        }
    }
    if (n == 0) { warn("%d taxids loaded", 0); return 0; }
    vector<u64> out(n), off;
    vector<u32> gt;
    {
        Gpu g(o.gpu);
        u64 groups = 0;
        ck(call_sized(UKM_ERR_CAPACITY, &groups, [&](u64 cap, u64 *m) {
            if (!cap) return ukm_tsplit(g.c, in.codes.data(), in.taxids.data(), n, nullptr, 0, nullptr, nullptr, 0, m);
            gt.resize(cap); off.resize(cap + 1);
            return ukm_tsplit(g.c, in.codes.data(), in.taxids.data(), n, out.data(), n, gt.data(), off.data(), cap, m);
        }));
    }
    info("%llu taxids belonging to %zu taxids loaded", (unsigned long long)n, gt.size());
    const u32 max_taxid = in.taxid_bytes >= 4 ? 0xFFFFFFFFu : ((1u << (8 * in.taxid_bytes)) - 1);  // maxUint32N: follow the readers
    for (size_t gi = 0; gi < gt.size(); gi++) {
        const string file = outdir + "/" + prefix + ".taxid-" + std::to_string(gt[gi]) + ".k" + std::to_string(h0.k) + EXT;
        write_unik(file, o, h0.k, out_mode(h0, true, false, o), max_taxid, gt[gi], nullptr, out.data() + off[gi], nullptr, off[gi + 1] - off[gi]);
    }
    info("%llu taxids belonging to %zu taxids saved to dir: %s", (unsigned long long)n, gt.size(), outdir.c_str());
    return 0;
}

static int cmd_grep(int argc, char **argv) {  // grep.go:62-890
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'q', "query", true}, {'f', "query-file", true}, {'F', "query-unik-file", true},
                                     {'t', "query-is-taxid", false}, {'D', "degenerate", false}, {'v', "invert-match", false}, {'s', "sort", false},
                                     {'u', "unique", false}, {'d', "repeated", false}, {'m', "multiple-outfiles", false}, {'O', "out-dir", true},
                                     {'S', "out-suffix", true}, {0, "force", false}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const vector<string> queries = a.list("query"), query_files = a.list("query-file"), query_unik_files = a.list("query-unik-file");
    const bool by_taxid = a.has("query-is-taxid"), invert = a.has("invert-match"), degenerate = a.has("degenerate");
    const bool uniq = a.has("unique"), rep = a.has("repeated");
    bool sort_kmers = a.has("sort");
    if ((uniq || rep) && !sort_kmers) {
        info("flag -s/--sort is switched on when given -u/--unique or -d/--repeated");
        sort_kmers = true;
    }
    if (queries.empty() && query_files.empty() && query_unik_files.empty())
        die("one of flags -q/--query, -f/--query-file and -F/--query-unik-file needed");
    if (a.has("multiple-outfiles") || a.has("out-dir") || a.has("out-suffix") || a.has("force"))
        die("flag -m/--multiple-outfiles (and -O/--out-dir, -S/--out-suffix, --force) is not supported in this build: run grep once per input file");
    int k = -1;
    // text queries from -q and -f (grep.go:122-166)
    vector<string> query_list;
    auto add_query = [&](const string &q) {
        if (!by_taxid) {
            if (k == -1) k = (int)q.size();
            else if ((int)q.size() != k) die("length of query sequence are inconsistent: (%zu) != (%d): %s", q.size(), k, q.c_str());
        }
        query_list.push_back(q);
    };
    for (auto &q : queries) if (!q.empty()) add_query(q);
    for (auto &qf : query_files) {
        info("loading queries from k-mer file: %s", qf.c_str());
        std::istringstream ss(read_text(qf));
        string line;
        while (std::getline(ss, line)) {
            trim_line_end(line);
            if (!line.empty()) add_query(line);
        }
    }
    vector<u64> q_codes;
    vector<u32> q_taxids;
    vector<string> q_text;  // k-mer text, encoded once the inputs say how (every query is searched: grep.go:173-190 keeps the last one only)
    for (auto &q : query_list) {
        if (by_taxid) {
            char *e = nullptr;
            errno = 0;
            const unsigned long long v = strtoull(q.c_str(), &e, 10);
            if (e == q.c_str() || *e || errno || v < 1 || v > 0xFFFFFFFFull || q[0] == '-')
                die("query taxid should be positive integer in range of [1, %u]: %s", 0xFFFFFFFFu, q.c_str());
            q_taxids.push_back((u32)v);
        } else if (degenerate) {
            for (auto &sq : extend_degenerate(q)) q_text.push_back(sq);
        } else {
            q_text.push_back(q);
        }
    }
    // queries from .unik files (grep.go:207-270)
    unik::Header qh0;
    bool have_qh0 = false;
    for (auto &qf : query_unik_files) {
        info("loading queries from .unik file: %s", qf.c_str());
        Options oo = o;
        oo.ignore_taxid = false;
        Loaded Q = load_unik(qf, oo);
        if (by_taxid && !Q.h.has_taxid_info()) die("no taxids found in file: %s", qf.c_str());
        if (!have_qh0) {
            if (k != -1) {
                if (k != Q.h.k) die("k-mer length not consistent (%d != %d), please check with \"unikmer stats\": %s", k, Q.h.k, qf.c_str());
            } else k = Q.h.k;
            qh0 = Q.h;
            have_qh0 = true;
        } else check_compat(qh0, Q.h, qf);
        if (by_taxid) {
            if (Q.per_record()) q_taxids.insert(q_taxids.end(), Q.taxids.begin(), Q.taxids.end());
            else if (!Q.codes.empty()) q_taxids.push_back(Q.file_taxid);
            continue;
        }
        const bool make_canonical = !Q.h.is_canonical() && !Q.h.is_hashed();
        for (u64 c : Q.codes) q_codes.push_back(make_canonical ? std::min(c, revcomp(c, Q.h.k)) : c);
    }
    // the inputs: compatible with the query files and with each other, same taxid situation (grep.go:439-441,550-563)
    Inputs in = load_inputs(files, o, LoadRules());
    if (have_qh0) check_compat(qh0, in.h0, files[0]);
    if (!by_taxid && k != in.k) die("K (%d) of binary file '%s' not equal to query K (%d)", in.k, files[0].c_str(), k);
    const bool tax = in.has_taxid;
    if ((uniq || rep) && tax)
        die("flag -u/--unique and -d/--repeated are not supported for inputs with taxids in this build (which duplicate's taxid the "
            "reference keeps is not defined); add -I/--ignore-taxid");
    if (by_taxid && !in.files.empty() && !in.h0.has_taxid_info()) info("the inputs carry no taxids: every record has taxid 0");
    if (!by_taxid && !in.hashed)
        for (auto &q : q_text) {
            u64 c;
            if (!encode_kmer(q, c)) die("fail to encode query '%s'", q.c_str());
            q_codes.push_back(std::min(c, revcomp(c, (int)q.size())));
        }
    const string out_file = out_name(a.str("out-prefix", "-"));
    // "forcing using canonical" (grep.go:499); one sorted input stays sorted
    const u32 mode = unik::UnikCanonical | out_mode(in.h0, sort_kmers || (files.size() == 1 && in.h0.is_sorted()), tax, o);

    vector<u64> codes;
    vector<u32> taxids;
    if (in.total) {
        Gpu g(o.gpu);
        if (!by_taxid && in.hashed && !q_text.empty()) {  // ntHash with the FILE's canonical flag, one window per query (grep.go:452-460)
            vector<u64> hv;
            hash_kmers_on_device(g, q_text, k, in.canonical, hv);
            q_codes.insert(q_codes.end(), hv.begin(), hv.end());
        }
        if (by_taxid) info("%zu taxids loaded", q_taxids.size());
        else info("%zu k-mers loaded", q_codes.size());
        const int canonical_k = (!in.canonical && !in.hashed) ? in.k : 0;
        const u64 nq = by_taxid ? q_taxids.size() : q_codes.size();
        // records of several inputs in FILE order
        select_per_file(in, tax, codes, taxids, [&](const Loaded &L, const u32 *own, u64 *ok, u32 *ot, u64 cap, u64 *n) {
            return ukm_grep(g.c, L.codes.data(), own, tax ? L.file_taxid : 0u, L.codes.size(), canonical_k, by_taxid ? nullptr : q_codes.data(),
                            by_taxid ? q_taxids.data() : nullptr, nq, (invert ? UKM_F_INVERT : 0u) | (by_taxid ? UKM_F_QUERY_TAXID : 0u), ok, ot, cap, n);
        });
        if (sort_kmers && !codes.empty()) {  // grep.go:790-875
            const int key_bits = in.hashed ? 64 : 2 * in.k;
            info("sorting %zu k-mers", codes.size());
            if (uniq || rep) {  // (never with taxids: refused above)
                vector<u64> u(codes.size());
                u.resize(sort_then_unique(g, codes.data(), nullptr, codes.size(), key_bits, uniq ? UKM_UNIQUE : UKM_REPEATED, u.data(), nullptr, u.size()));
                codes.swap(u);
            } else {
                sort_records(g, codes.data(), tax ? taxids.data() : nullptr, codes.size(), key_bits);
            }
        }
    }
    write_following(out_file, o, in.h0, mode, codes.data(), taxids.data(), codes.size());
    return 0;
}
