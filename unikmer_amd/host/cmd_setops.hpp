// cmd_setops.hpp — union / inter / diff / common: n-way set operations over whole files
#pragma once
#include <iostream>

#include "records.hpp"

enum SetOp { OP_UNION, OP_INTER, OP_DIFF, OP_COMMON };
static const vector<FlagSpec> SETOP_FLAGS[] = {
    /* union  */ {{'o', "out-prefix", true}, {'s', "sort", false}},
    /* inter  */ {{'o', "out-prefix", true}, {'m', "mix-taxid", false}},
    /* diff   */ {{'o', "out-prefix", true}, {'s', "sort", false}, {'t', "compare-taxid", false}},
    /* common */ {{'o', "out-prefix", true}, {'m', "mix-taxid", false}, {'p', "proportion", true}, {'n', "number", true}},
};

static int cmd_setop(SetOp which, int argc, char **argv) {
    Args a = parse_args(argc, argv, SETOP_FLAGS[which]);
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const string out_file = out_name(a.str("out-prefix", "-"));
    const bool mix = a.has("mix-taxid");

    // single-input fast path of union / inter: the file is copied byte for byte (union.go:97-112, inter.go:96-120)
    if ((which == OP_UNION || which == OP_INTER) && files.size() == 1 && files[0] != "-") {
        if (which == OP_INTER) { unik::Reader r(files[0]); if (!r.h.is_sorted() && !a.has("skip-flag-check")) die("input should be sorted: %s", files[0].c_str()); }
        std::ifstream src(files[0], std::ios::binary);
        if (out_file == "-") std::cout << src.rdbuf();
        else { std::ofstream dst(out_file, std::ios::binary); dst << src.rdbuf(); }
        return 0;
    }

    LoadRules rules;
    rules.tax = mix ? LoadRules::MIX : LoadRules::SAME;
    if (which == OP_INTER && !a.has("skip-flag-check")) rules.sorted = LoadRules::ALL;
    if (which == OP_DIFF) { rules.sorted = LoadRules::FIRST; rules.unsorted = "the first file should be sorted: %s"; }
    Inputs in = load_inputs(files, o, rules);
    const bool tax = in.has_taxid || (mix && in.any_taxid);  // (diff has no -m: taxid always from file 1, diff.go:496-515)
    Gpu g(o.gpu);
    u32 max_taxid = o.max_taxid;
    bool cmp_taxid = which == OP_DIFF && a.has("compare-taxid");
    if (cmp_taxid && !in.has_taxid) {  // diff.go:124-133: a warning, the flag is ignored
        fprintf(stderr, "[WARN] no taxids found in the first file, flag -t/--compare-taxid ignored\n");
        cmp_taxid = false;
    }
    if ((tax && which != OP_DIFF) || cmp_taxid) max_taxid = load_taxonomy(g, o);
    const bool with_t = tax || cmp_taxid;
    Ptrs p = ptrs_of(in, with_t);
    const int ns = (int)in.files.size();
    const u64 cap = which == OP_INTER || which == OP_DIFF ? in.files[0].codes.size() : in.total;
    vector<u64> out(cap ? cap : 1);
    vector<u32> tout(with_t ? (cap ? cap : 1) : 0);
    u64 n = 0;
    const u32 *const *tp = with_t ? p.t.data() : nullptr;
    const u32 *fp = with_t ? p.ft.data() : nullptr;
    u32 *to = with_t ? tout.data() : nullptr;
    bool sorted_out = true;
    switch (which) {
    case OP_UNION:
        ck(ukm_union_ft(g.c, p.k.data(), tp, fp, p.n.data(), ns, 0, out.data(), to, cap, &n));
        sorted_out = a.has("sort");  // same stream; the flag/encoding follow -s (union.go:220-235)
        break;
    case OP_INTER:
        ck(ukm_inter_ft(g.c, p.k.data(), tp, fp, p.n.data(), ns, mix ? UKM_F_MIX_TAXID : 0, out.data(), to, cap, &n));
        if (n == 0) info("no intersection found");
        break;
    case OP_DIFF: {
        // files equal (by path) to the first one are skipped (diff.go:464-466)
        Ptrs q; vector<uint8_t> sf;
        for (int i = 0; i < ns; i++) if (i == 0 || files[(size_t)i] != files[0]) { q.k.push_back(p.k[(size_t)i]); q.t.push_back(p.t[(size_t)i]); q.ft.push_back(p.ft[(size_t)i]); q.n.push_back(p.n[(size_t)i]); sf.push_back(in.files[(size_t)i].h.is_sorted() ? 1 : 0); }
        ck(ukm_diff_ft(g.c, q.k.data(), with_t ? q.t.data() : nullptr, with_t ? q.ft.data() : nullptr, q.n.data(), (int)q.k.size(), sf.data(),
                       cmp_taxid ? UKM_F_CMP_TAXID : 0, out.data(), to, cap, &n));
        if (n == 0) fprintf(stderr, "[WARN] no set difference found\n");
        sorted_out = a.has("sort");
        break;
    }
    case OP_COMMON: {
        const double prop = a.real("proportion", 1.0);
        if (prop <= 0 || prop > 1) die("value of -p/--proportion should be in range of (0, 1]");
        if (ns > 65535) die("at most 65535 files supported");
        const u32 thr = ukm_common_threshold((u32)ns, prop, (u32)a.num("number", 0));
        info("searching k-mers shared by >= %u files ...", thr);
        ck(ukm_common_ft(g.c, p.k.data(), tp, fp, p.n.data(), ns, thr, 0, out.data(), to, cap, &n));
        break;
    }
    }
    // a global taxid shared by every input survives as the header's global taxid when no per-record taxids are written
    write_unik(out_file, o, in.k, out_mode(in.h0, sorted_out, tax, o), max_taxid, 0, &in.h0, out.data(), tax ? tout.data() : nullptr, n);
    return 0;
}
