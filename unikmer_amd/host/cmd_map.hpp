// cmd_map.hpp — locate / map (uniqs): k-mers back to genome coordinates (ukm_locate / ukm_map)
#pragma once
#include <regex>

#include "records.hpp"

// genome records with their ids; -B/--seq-name-filter drops records by name, case ignored (locate.go:60-71,176-187)
struct GenomeSink : FastxSink {
    SeqBatch &b;
    const vector<std::regex> &skip;
    GenomeSink(SeqBatch &bb, const vector<std::regex> &sk) : b(bb), skip(sk) {}
    bool begin_record(const string &name) override {
        for (auto &re : skip) if (std::regex_search(name, re)) return false;
        b.names.push_back(name.substr(0, name.find_first_of(" \t")));  // record.ID
        return true;
    }
    void add_seq(const char *p, size_t n) override { b.bases.insert(b.bases.end(), p, p + n); }
    void end_record() override { b.off.push_back(b.bases.size()); }
};
static vector<std::regex> name_filters(const Args &a) {
    vector<std::regex> out;
    for (auto &kw : a.list("seq-name-filter")) {
        try { out.emplace_back(kw, std::regex::icase); }
        catch (const std::regex_error &) { die("failed to parse regular expression for matching sequence header: %s", kw.c_str()); }
    }
    return out;
}
// the .unik inputs of both commands: same k and flags, canonical (locate.go:126-136, map.go:141-151); concat: the codes in file order
static Inputs load_canonical_inputs(const vector<string> &files, const Options &o, bool concat) {
    Options oo = o;
    oo.ignore_taxid = true;
    LoadRules rules;
    rules.tax = LoadRules::MIX;
    rules.concat = concat;
    Inputs in = load_inputs(files, oo, rules);
    if (!in.canonical) die("%s: 'canonical' flag is needed", files[0].c_str());
    return in;
}

static int cmd_locate(int argc, char **argv) {  // locate.go:57-289
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'g', "genome", true}, {'B', "seq-name-filter", true}, {0, "circular", false}});
    Options o = get_options(a);
    const vector<string> genomes = a.list("genome");
    if (genomes.empty()) die("flag -g/--genome needed");
    const vector<std::regex> skip = name_filters(a);
    vector<string> files = get_files(a, o);
    if (files.size() == 1 && files[0] == "-") die("stdin not supported, please give me .unik files");
    const bool circular = a.has("circular");
    Inputs in = load_canonical_inputs(files, o, true);
    const int k = in.k;
    const vector<u64> &q = in.codes;
    SeqBatch gb;
    GenomeSink sink(gb, skip);
    for (auto &gf : genomes) { info("reading genome file: %s", gf.c_str()); parse_fastx(gf, sink); }
    const u64 n_rec = gb.off.size() - 1;
    auto out = text_out(a.str("out-prefix", "-"));
    if (n_rec == 0 || q.empty()) { out->close(); return 0; }
    Gpu g(o.gpu);
    vector<u64> oq, opos;
    vector<u32> orec;
    u64 n = 0;
    ck(call_grow(UKM_ERR_CAPACITY, std::max<u64>(1u << 16, 2 * q.size()), &n, [&](u64 cap, u64 *m) {
        oq.resize(cap); opos.resize(cap); orec.resize(cap);
        return ukm_locate(g.c, gb.bases.data(), gb.off.data(), n_rec, k, circular, in.hashed, q.data(), q.size(), oq.data(), orec.data(), opos.data(), cap, m);
    }));
    string buf;
    for (u64 e = 0; e < n; e++) {
        const u64 r = orec[e], j = opos[e], rs = gb.off[r], len = gb.off[r + 1] - rs;
        buf += gb.names[r]; buf += '\t'; buf += std::to_string(j); buf += '\t'; buf += std::to_string(j + (u64)k); buf += '\t';
        for (u64 t = j; t < j + (u64)k; t++) buf += (char)gb.bases[rs + (t < len ? t : t - len)];  // (circular: the record extended by its first k - 1 bases)
        buf += "\t0\t.\n";
        if (buf.size() > (1u << 20)) { put(*out, buf); buf.clear(); }
    }
    put(*out, buf);
    out->close();
    return 0;
}

static int cmd_map(int argc, char **argv) {  // map.go:57-491 at -x 0 -X 0, linear genomes
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'g', "genome", true}, {'B', "seq-name-filter", true}, {'m', "min-len", true},
                                     {'M', "allow-multiple-mapped-kmers", false}, {'W', "seqs-in-a-file-as-one-genome", false},
                                     {'a', "output-fasta", false}, {'x', "max-gap-size", true}, {'X', "max-gap-num", true}, {0, "circular", false}});
    Options o = get_options(a);
    const vector<string> genomes = a.list("genome");
    if (genomes.empty()) die("flag -g/--genome needed");
    const long long min_len = a.num("min-len", 200);
    if (min_len <= 0) die("value of flag --min-len should be greater than 0");
    const bool multi = a.has("allow-multiple-mapped-kmers"), one_genome = a.has("seqs-in-a-file-as-one-genome"), fasta = a.has("output-fasta");
    if (one_genome && multi) die("flag -M/--allow-multiple-mapped-kmers and -W/--seqs-in-a-file-as-one-genome are not compatible");
    if (a.num("max-gap-size", 0) < 0 || a.num("max-gap-num", 0) < 0) die("value of flag -x/--max-gap-size and -X/--max-gap-num should be >= 0");
    if (a.num("max-gap-size", 0) > 0 || a.num("max-gap-num", 0) > 0)
        die("flag -x/--max-gap-size and -X/--max-gap-num above 0 are not supported in this build (regions are runs of consecutive mapped k-mers)");
    if (a.has("circular")) die("flag --circular is not supported by map in this build");
    const vector<std::regex> skip = name_filters(a);
    vector<string> files = get_files(a, o);
    Inputs in = load_canonical_inputs(files, o, false);
    const int k = in.k;
    auto out = text_out(a.str("out-prefix", "-"));
    Gpu g(o.gpu);
    // the set: the union of all input files, built and kept on the device
    DevMem set(g.c, std::max<u64>(in.total, 1) * sizeof(u64));
    u64 n_set = 0;
    {
        Ptrs p = ptrs_of(in, false);
        ck(ukm_union(g.c, p.k.data(), nullptr, p.n.data(), (int)p.k.size(), 0, (u64 *)set.p, nullptr, in.total, &n_set));
        info("%llu k-mers loaded", (unsigned long long)n_set);
    }
    // genomes one file at a time; with -W the reference never advances its genome index, so all files are ONE genome
    vector<SeqBatch> batches;
    for (auto &gf : genomes) {
        if (batches.empty() || !one_genome) batches.emplace_back();
        info("reading genome file: %s", gf.c_str());
        GenomeSink sink(batches.back(), skip);
        parse_fastx(gf, sink);
    }
    string buf;
    for (auto &gb : batches) {
        const u64 n_rec = gb.off.size() - 1;
        if (n_rec == 0) continue;
        vector<u64> goff;
        if (one_genome) goff = {0, n_rec};
        else for (u64 r = 0; r <= n_rec; r++) goff.push_back(r);  // one genome per record (the first pass's numbering, map.go:260-262)
        vector<u32> orec;
        vector<u64> os, oe;
        u64 n = 0;
        ck(call_grow(UKM_ERR_CAPACITY, 1u << 16, &n, [&](u64 cap, u64 *m) {
            orec.resize(cap); os.resize(cap); oe.resize(cap);
            return ukm_map(g.c, gb.bases.data(), gb.off.data(), n_rec, goff.data(), goff.size() - 1, k, in.hashed, (const u64 *)set.p, n_set,
                           multi, (u64)min_len, orec.data(), os.data(), oe.data(), cap, m);
        }));
        for (u64 e = 0; e < n; e++) {
            const u64 r = orec[e], rs = gb.off[r];
            if (fasta) {  // map.go:385-387: >id:start+1-end, the subsequence wrapped at 60
                buf += '>'; buf += gb.names[r]; buf += ':'; buf += std::to_string(os[e] + 1); buf += '-'; buf += std::to_string(oe[e]); buf += '\n';
                for (u64 t = os[e]; t < oe[e]; t += 60) {
                    buf.append((const char *)gb.bases.data() + rs + t, (size_t)std::min<u64>(60, oe[e] - t));
                    buf += '\n';
                }
            } else {
                buf += gb.names[r]; buf += '\t'; buf += std::to_string(os[e]); buf += '\t'; buf += std::to_string(oe[e]); buf += '\n';
            }
            if (buf.size() > (1u << 20)) { put(*out, buf); buf.clear(); }
        }
    }
    put(*out, buf);
    out->close();
    return 0;
}
