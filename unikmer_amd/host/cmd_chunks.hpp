// cmd_chunks.hpp — sort / split / merge and their out-of-core chunk protocol
// (sort.go:241-447, split.go:288-401, merge.go:228-341)
#pragma once
#include <regex>

#include "records.hpp"

struct ChunkJob {
    int k = 0;
    u32 mode = 0;  // includes UnikSorted
    bool tax = false, uniq = false, rep = false;
    int key_bits = 64;
    u32 max_taxid = 0xFFFFFFFFu;
    const unik::Header *h0 = nullptr;
};
// one chunk: device sort + the scan of dumpCodes2File / dumpCodesTaxids2File (util-sort.go:35-190):
// -u collapses runs (LCA of their taxids), -d writes every code once and repeated ones twice, else plain
static u64 sort_chunk_to_file(Gpu &g, const Options &o, const ChunkJob &j, u64 *codes, u32 *taxids, u64 n, const string &file) {
    vector<u64> out(2 * n + 1);
    vector<u32> tout(j.tax ? 2 * n + 1 : 0);
    const u64 m = sort_then_unique(g, codes, j.tax ? taxids : nullptr, n, j.key_bits, j.uniq ? UKM_UNIQUE : (j.rep ? UKM_REPEATED_CHUNK : UKM_PLAIN),
                                   out.data(), tout.data(), 2 * n + 1);
    write_unik(file, o, j.k, j.mode, j.max_taxid, 0, j.h0, out.data(), j.tax ? tout.data() : nullptr, m);
    return m;
}

// mergeChunksFile (util-sort.go:227-606) over sorted chunk files, on the device.  Files are loaded
// whole (HBM holds far more than the reference's open-file budget); when there are at least
// `max_open` of them the reference's two rounds are kept: groups of max_open files are merged with
// finalRound = false into new chunk files, then those are merged with finalRound = true.
static u64 merge_files_once(Gpu &g, const Options &o, const ChunkJob &j, const vector<string> &files, const string &out_file, bool final_round) {
    Options oo = o;
    oo.ignore_taxid = !j.tax;
    LoadRules rules;
    rules.against = j.h0;
    rules.announce = false;
    rules.sorted = LoadRules::ALL; rules.unsorted = "chunk file should be sorted: %s"; rules.sorted_before_taxid = true;
    rules.tax = j.tax ? LoadRules::EVERY : LoadRules::MIX;
    rules.no_taxid = "taxid information found in previous files, but missing in this: %s";
    Inputs in = load_inputs(files, oo, rules);
    Ptrs p = ptrs_of(in, j.tax);
    const u64 cap = 2 * in.total + 1;
    vector<u64> out(cap);
    vector<u32> tout(j.tax ? cap : 0);
    u64 n = 0;
    if (!in.files.empty())
        ck(ukm_merge_k_ft(g.c, p.k.data(), j.tax ? p.t.data() : nullptr, j.tax ? p.ft.data() : nullptr, p.n.data(), (int)in.files.size(),
                          j.uniq ? UKM_UNIQUE : (j.rep ? UKM_REPEATED : UKM_PLAIN), final_round ? 1 : 0, out.data(), j.tax ? tout.data() : nullptr, cap, &n));
    write_unik(out_file, o, j.k, j.mode, j.max_taxid, 0, j.h0, out.data(), j.tax ? tout.data() : nullptr, n);
    return n;
}
static u64 merge_rounds(Gpu &g, const Options &o, const ChunkJob &j, vector<string> files, const string &out_file, int max_open,
                        const string &tmp_dir, int &i_tmp, vector<string> &made) {
    if ((int)files.size() < max_open) {
        info("======= Stage 2: merging from %zu chunks =======", files.size());
        return merge_files_once(g, o, j, files, out_file, true);
    }
    info("======= Stage 2: merging from %zu chunks (round: 1/2) =======", files.size());
    vector<string> next, group;
    auto flush = [&]() {
        if (group.empty()) return;
        const string f = chunk_file_name(tmp_dir, ++i_tmp);
        info("[chunk %d] sorting k-mers from %zu tmp files", i_tmp, group.size());
        merge_files_once(g, o, j, group, f, false);
        next.push_back(f);
        made.push_back(f);
        group.clear();
    };
    for (auto &f : files) { group.push_back(f); if ((int)group.size() == max_open) flush(); }
    flush();
    info("======= Stage 3: merging from %zu chunks (round: 2/2) =======", next.size());
    return merge_files_once(g, o, j, next, out_file, true);
}
static string tmp_dir_for(const string &tmp_root, const string &out_prefix) {  // sort.go:113-118
    const string root = tmp_root.empty() ? string("./") : tmp_root;
    return root + (root.back() == '/' ? "" : "/") + (out_prefix == "-" ? string("stdout.tmp") : base_of(out_prefix) + ".tmp");
}
static void cleanup_tmp(const vector<string> &files, const string &dir, bool keep) {  // sort.go:425-446
    if (keep) return;
    info("removing %zu intermediate files", files.size());
    for (auto &f : files) if (remove(f.c_str()) != 0) die("fail to remove intermediate file: %s", f.c_str());
    info("removing tmp dir: %s", dir.c_str());
    if (rmdir(dir.c_str()) != 0) die("fail to remove temp directory, please manually delete it: %s", dir.c_str());
}

enum ChunkCmd { CH_SORT, CH_SPLIT, CH_MERGE };
static const vector<FlagSpec> CHUNK_FLAGS[] = {
    /* sort  */ {{'o', "out-prefix", true}, {'u', "unique", false}, {'d', "repeated", false}, {'M', "max-open-files", true}, {'t', "tmp-dir", true},
                 {'k', "keep-tmp-dir", false}, {0, "force", false}, {'m', "chunk-size", true}},
    /* split */ {{'O', "out-dir", true}, {'m', "chunk-size", true}, {0, "force", false}, {'u', "unique", false}, {'d', "repeated", false}},
    /* merge */ {{'o', "out-prefix", true}, {'u', "unique", false}, {'d', "repeated", false}, {'M', "max-open-files", true}, {'t', "tmp-dir", true},
                 {'k', "keep-tmp-dir", false}, {0, "force", false}, {'D', "is-dir", false}, {'p', "pattern", true}},
};

static int cmd_chunks(ChunkCmd which, int argc, char **argv) {
    Args a = parse_args(argc, argv, CHUNK_FLAGS[which]);
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const string out_prefix = a.str("out-prefix", "-");
    const string out_file = out_name(out_prefix);
    ChunkJob j;
    j.uniq = a.has("unique"); j.rep = a.has("repeated");
    if (j.uniq && j.rep) die("flag -u/--unique overides -d/--repeated, do not give both");
    const int max_open = (int)a.num("max-open-files", 400);
    if (max_open <= 0) die("value of flag --max-open-files should be positive");

    if (which == CH_MERGE) {  // merge.go:228-341
        if (a.has("is-dir")) {  // merge.go:77-130: chunk files of the given directories
            std::regex re(a.str("pattern", "^chunk_\\d+\\.unik$"));
            vector<string> found;
            for (auto d : files) {
                if (d == "-") d = "./";
                if (!dir_exists(d)) { fprintf(stderr, "[WARN] skip unexisted dir: %s\n", d.c_str()); continue; }
                size_t nf = 0;
                for (auto &nme : list_dir(d)) {
                    if (nme[0] == '.' || dir_exists(d + "/" + nme) || !std::regex_search(nme, re)) continue;
                    found.push_back(d + (d.back() == '/' ? "" : "/") + nme);
                    nf++;
                }
                info("%zu chunk files found in dir: %s", nf, d.c_str());
            }
            if (found.empty()) { fprintf(stderr, "[WARN] 0 chunk files found in %zu dir(s)\n", files.size()); return 0; }
            files = found;
        }
        unik::Reader r0(files[0]);
        j.k = r0.h.k; j.h0 = &r0.h;
        j.tax = !o.ignore_taxid && r0.h.has_taxid_info();
        j.key_bits = r0.h.is_hashed() ? 64 : 2 * r0.h.k;
        j.mode = out_mode(r0.h, true, j.tax, o);
        Gpu g(o.gpu);
        j.max_taxid = j.tax && (j.uniq || j.rep) ? load_taxonomy(g, o) : o.max_taxid;
        vector<string> made;
        int i_tmp = 0;
        string tmp_dir;
        if ((int)files.size() >= max_open) {
            tmp_dir = tmp_dir_for(a.str("tmp-dir", "./"), out_prefix);
            prepare_dir(tmp_dir, a.has("force"), "tmp dir");
        }
        merge_rounds(g, o, j, files, out_file, max_open, tmp_dir, i_tmp, made);
        if (!tmp_dir.empty()) cleanup_tmp(made, tmp_dir, a.has("keep-tmp-dir"));
        return 0;
    }

    // sort.go:227-572.  Without -m (or when the input is smaller than one chunk) everything is
    // sorted in HBM in one go; with -m N the reference's chunk protocol runs: stage 1 sorts
    // chunks of N k-mers into tmp files (-u: deduplicated, -d: every code once and repeated ones
    // twice), stage 2/3 merge them (merge_rounds).  `split` is stage 1 alone (split.go).
    LoadRules rules;
    rules.concat = true;  // one sort over all inputs, or over slices of them: the array is what it takes
    Inputs in = load_inputs(files, o, rules);
    j.tax = in.has_taxid;
    Gpu g(o.gpu);
    j.max_taxid = j.tax && (j.uniq || j.rep) ? load_taxonomy(g, o) : o.max_taxid;  // sort.go:196-198
    j.k = in.k; j.h0 = &in.h0;
    j.key_bits = in.hashed ? 64 : 2 * in.k;
    j.mode = out_mode(in.h0, true, j.tax, o);
    u32 *taxids = j.tax ? in.taxids.data() : nullptr;
    const long long max_elem = parse_byte_size(a.str("chunk-size", ""));
    if (which == CH_SPLIT || (max_elem > 0 && in.total >= (u64)max_elem)) {
        string dir;
        if (which == CH_SPLIT) {
            dir = a.str("out-dir", "");
            if (dir.empty()) dir = (files[0] == "-" ? string("stdin") : files[0]) + ".split";
            if (dir != "./" && dir != ".") prepare_dir(dir, a.has("force"), "outDir");
        } else {
            dir = tmp_dir_for(a.str("tmp-dir", "./"), out_prefix);
            prepare_dir(dir, a.has("force"), "tmp dir");
            info("======= Stage 1: spliting k-mers into chunks =======");
        }
        const u64 step = max_elem > 0 ? (u64)max_elem : (in.total ? in.total : 1);
        vector<string> chunks;
        int i_tmp = 0;
        for (u64 b = 0; b < in.total; b += step) {
            const u64 cn = std::min(step, in.total - b);
            const string f = chunk_file_name(dir, ++i_tmp);
            info("[chunk %d] sorting %zu k-mers", i_tmp, (size_t)cn);
            const u64 m = sort_chunk_to_file(g, o, j, in.codes.data() + b, j.tax ? taxids + b : nullptr, cn, f);
            info("[chunk %d] %llu k-mers saved to tmp file: %s", i_tmp, (unsigned long long)m, f.c_str());
            chunks.push_back(f);
        }
        if (which == CH_SPLIT) { info("%llu k-mers saved to %zu chunk files in %s", (unsigned long long)in.total, chunks.size(), dir.c_str()); return 0; }
        vector<string> made = chunks;
        merge_rounds(g, o, j, chunks, out_file, max_open, dir, i_tmp, made);
        cleanup_tmp(made, dir, a.has("keep-tmp-dir"));
        return 0;
    }
    const u64 cap = 2 * in.total;
    vector<u64> out(cap ? cap : 1);
    vector<u32> tout(j.tax ? (cap ? cap : 1) : 0);
    const u64 n = sort_then_unique(g, in.codes.data(), taxids, in.total, j.key_bits, j.uniq ? UKM_UNIQUE : (j.rep ? UKM_REPEATED : UKM_PLAIN),
                                   out.data(), tout.data(), cap);
    write_unik(out_file, o, in.k, j.mode, j.max_taxid, 0, &in.h0, out.data(), j.tax ? tout.data() : nullptr, n);
    return 0;
}
