// cmd_count.hpp — `count` (count.go:41-602): the device stages of its chunk pipeline (count_pipe.hpp) and the command
#pragma once
#include <ctime>

#include "count_pipe.hpp"
#include "records.hpp"

// ---- count: device-resident pipeline ------------------------------------------------------------------------
// FASTA/Q bases go to the GPU in chunks through page-locked staging buffers: chunk i+1 is uploaded on the context's
// transfer stream while chunk i is encoded / hashed (count.go:285-299 reads record by record; here a "record batch" is a
// chunk).  The window values never come back to the host: they are written to ONE device array, sorted and reduced there
// (count.go:424-436, 571-581), and only the final set crosses PCIe.  The threads, the chunks and the loop are
// count_pipe.hpp's; here are the two stages the loop drives -- chunks parsed on the host (ParsedStage), raw chunks parsed
// by ukm_fastx (RawStage) --, what both append to (Windows) and the sort + unique behind them (finish_count).
static double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
// what is counted, and how the input gets to the device
struct CountJob {
    int k = 0;
    bool canonical = false, circular = false, hashed = false;
    u64 max_hash = 0;       // --scale: hashes above it are dropped (0: none)
    int minimizer_w = 0;    // -W (0: every window)
    bool linear = false;    // -l: no sort, no unique
    int uniq_mode = UKM_UNIQUE, key_bits = 64;
    const std::regex *skip_name = nullptr, *tax_re = nullptr;  // -B; -T -r
    bool device_fastx = false, fastx_report = false;
    u64 chunk_bytes = 32u << 20;
};

// What both stages append to: the windows of every chunk in ONE growing device array; with -T their taxids in a second.
struct Windows {
    Gpu &g;
    const CountJob &job;
    DevBuf codes, tax;
    u64 n = 0, total_bases = 0, nchunks = 0;
    Windows(Gpu &gg, const CountJob &j) : g(gg), job(j), codes(gg.c), tax(gg.c) {}
    // the windows of nrec records (nb bases; host or device pointers) behind the n there are: THE choice of the window kernel
    u64 append(const uint8_t *bases, const u64 *off, u64 nrec, u64 nb) {
        codes.ensure((n + nb) * 8, n * 8);  // windows <= bases
        u64 *dst = codes.as<u64>() + n;
        const u64 room = codes.cap / 8 - n;
        u64 m = 0;
        if (job.minimizer_w > 0) ck(ukm_minimizer(g.c, bases, off, nrec, job.k, job.minimizer_w, job.circular, job.max_hash, dst, nullptr, room, &m));
        else if (job.hashed) ck(ukm_nthash(g.c, bases, off, nrec, job.k, job.canonical, job.circular, job.max_hash, dst, room, &m));
        else ck(ukm_encode_kmers(g.c, bases, off, nrec, job.k, job.canonical, job.circular, dst, room, &m));
        n += m;
        total_bases += nb;
        return m;
    }
};

// Chunks parsed on the host: bases + record offsets, with -T a taxid per window.
struct ParsedStage {
    Windows &w;
    ChunkPipe &pipe;
    struct Slot {
        DevBuf bases, off, tax;
        int host = -1;
        u64 nrec = 0;
        explicit Slot(ukm_ctx *c) : bases(c), off(c), tax(c) {}
    };
    Slot sl[2];
    ParsedStage(Windows &ww, ChunkPipe &p) : w(ww), pipe(p), sl{Slot(ww.g.c), Slot(ww.g.c)} {}
    void fence() { ck(ukm_copy_fence(w.g.c)); }
    void upload(int s, int hi) {
        Slot &d = sl[s];
        const HostChunk &h = pipe.chunk(hi);
        const u64 ob = h.off.size() * 8, tb = h.wtax.size() * 4;
        d.bases.ensure(h.nb);
        d.off.ensure(ob);
        ck(ukm_copy_async(w.g.c, d.bases.p, h.bases, h.nb));
        ck(ukm_copy_async(w.g.c, d.off.p, h.off.data(), ob));   // (pageable source: staged by the runtime)
        if (w.job.tax_re && tb) {
            d.tax.ensure(tb);
            ck(ukm_copy_async(w.g.c, d.tax.p, h.wtax.data(), tb));
        }
        d.host = hi;
        d.nrec = h.off.size() - 1;
        w.nchunks++;
    }
    void compute(int s, int, int &) {
        Slot &d = sl[s];
        const HostChunk &h = pipe.chunk(d.host);
        const u64 at = w.n, m = w.append(d.bases.p, d.off.as<u64>(), d.nrec, h.nb);
        if (w.job.tax_re) {
            if (m != h.wtax.size()) die("count -T: %llu windows but %zu taxids in a chunk", (unsigned long long)m, h.wtax.size());
            w.tax.ensure((at + m) * 4 + 8, at * 4);
            if (m) ck(ukm_copy(w.g.c, w.tax.as<u32>() + at, d.tax.p, m * 4));  // device to device, ordered behind the upload by the fence
        }
        pipe.put_free(d.host);  // its upload is complete (the kernels waited for it): the reader may refill it
        d.host = -1;
    }
};

// Raw chunks through ukm_fastx.  A slot holds a chunk's raw bytes behind `pad` bytes of room, into which the bytes the
// previous call left unconsumed (an incomplete record) are copied device to device: the text of a call is tail + chunk.
// What is outside the device's grammar goes to the host parser, with the rest of its file.
struct RawStage {
    Windows &w;
    ChunkPipe &pipe;
    const vector<string> &files;
    struct Slot {
        DevBuf text;
        u64 pad = 0, nb = 0;
        int host = -1;
        explicit Slot(ukm_ctx *c) : text(c) {}
    };
    Slot sl[2];
    DevBuf bases, rec;                    // what ukm_fastx writes: the bases and the record offsets of a call
    u64 tail = 0, fpos = 0, fchunks = 0;  // unconsumed bytes in front of the current chunk and the file offset they start at; the file's chunks so far
    RawStage(Windows &ww, ChunkPipe &p, const vector<string> &f)
        : w(ww), pipe(p), files(f), sl{Slot(ww.g.c), Slot(ww.g.c)}, bases(ww.g.c), rec(ww.g.c) {}
    void fence() { ck(ukm_copy_fence(w.g.c)); }
    // at least `pad` bytes in front of `data` bytes; keeps the chunk in the slot.  The pad only grows.
    void room(Slot &d, u64 pad, u64 data) {
        const u64 have = d.text.p ? d.text.cap - d.pad : 0;
        if (d.text.p && d.pad >= pad && have >= data) return;
        ck(ukm_copy_sync(w.g.c));  // (an upload into the old buffer may be on its way)
        const u64 npad = d.text.p ? std::max<u64>((pad + pad / 2 + 15) & ~(u64)15, d.pad) : ((pad + 15) & ~(u64)15);
        DevBuf grown(w.g.c, npad + std::max(data, have));
        if (d.nb) ck(ukm_copy(w.g.c, grown.p + npad, d.text.p + d.pad, d.nb));
        d.text.swap(grown);
        d.pad = npad;
    }
    void upload(int s, int hi) {
        Slot &d = sl[s];
        const HostChunk &h = pipe.chunk(hi);
        room(d, 1 << 20, w.job.chunk_bytes);
        d.nb = h.nb;
        if (h.nb) ck(ukm_copy_async(w.g.c, d.text.p + d.pad, h.bases, h.nb));
        d.host = hi;
        w.nchunks++;
    }
    void compute(int s, int o, int &nxt) {
        Slot &d = sl[s];
        const HostChunk &h = pipe.chunk(d.host);
        const int fi = h.file;
        const bool last = h.last, fastq = h.fastq;
        if (h.first) { fpos = 0; fchunks = 0; }  // (records never span files: the tail is empty)
        fchunks++;
        const uint8_t *text = d.text.p + d.pad - tail;
        const u64 nt = tail + d.nb;
        u64 nb = 0, nrec = 0, used = 0;
        int stop = UKM_FASTX_STOP_NONE;
        if (nt) {
            bases.ensure(nt);                // the most a text can hold: every byte a base;
            rec.ensure((nt / 2 + 2) * 8);    // a record in two bytes, and the offsets' closing entry
            ck(ukm_fastx(w.g.c, text, nt, (fastq ? UKM_FASTX_FASTQ : 0u) | (last ? UKM_FASTX_LAST : 0u), bases.p, bases.cap,
                         rec.as<u64>(), nullptr, rec.cap / 8 - 1, &nb, &nrec, &used, &stop));
            if (nrec) w.append(bases.p, rec.as<u64>(), nrec, nb);
        }
        pipe.put_free(d.host);  // its upload is complete (the kernels waited for it): the reader may refill it
        d.host = -1;
        if (stop == UKM_FASTX_STOP_GRAMMAR) { to_host_parser(o, nxt, text + used, nt - used, fi, last, fastq, fpos + used); return; }
        tail = nt - used;
        fpos += used;
        if (tail) {  // in front of the next chunk, device to device (a record longer than the room: the room grows)
            room(sl[o], tail, w.job.chunk_bytes);
            ck(ukm_copy(w.g.c, sl[o].text.p + sl[o].pad - tail, text + used, tail));
        }
        if (last && w.job.fastx_report) fprintf(stderr, "fastx: %s: device, %llu chunk(s)\n", files[fi].c_str(), (unsigned long long)fchunks);
    }
    // Outside the device's grammar: the rest of file fi -- the n_left bytes at `left` on the device, the chunks already read,
    // the stream -- goes through the host parser, from a byte (`at` in the file) at which its state machine expects a header.
    // nxt, the chunk on its way to slot o, is the file's and is taken over: the next file's first chunk takes its place.
    void to_host_parser(int o, int &nxt, const uint8_t *left, u64 n_left, int fi, bool last, bool fastq, u64 at) {
        vector<char> mem(n_left);
        if (n_left) ck(ukm_copy(w.g.c, mem.data(), left, n_left));
        tail = 0;
        ChunkPipe::Rest rest;
        rest.exhausted = last;
        if (!last) {
            const bool on_its_way = nxt >= 0;
            if (on_its_way) { ck(ukm_copy_sync(w.g.c)); sl[o].host = -1; sl[o].nb = 0; }  // its upload ends before the reader may refill it
            rest = pipe.take_rest_of(fi, nxt);
            nxt = -1;
            mem.insert(mem.end(), rest.bytes.begin(), rest.bytes.end());
            vector<char>().swap(rest.bytes);
            fchunks += rest.chunks;
            w.nchunks += rest.chunks - (on_its_way ? 1 : 0);  // (that one was counted by its upload)
        }
        BatchFlushSink sink;
        sink.chunk_bytes = w.job.chunk_bytes;
        sink.out = [&](const uint8_t *b, const u64 *off, u64 nrec, u64 nb) { w.append(b, off, nrec, nb); };
        parse_fastx(mem.data(), mem.size(), rest.stream, fastq, files[fi], sink);
        sink.flush();
        pipe.release_reader();
        if (w.job.fastx_report)
            fprintf(stderr, "fastx: %s: device, %llu chunk(s), host from byte %llu (grammar)\n", files[fi].c_str(), (unsigned long long)fchunks,
                    (unsigned long long)at);
        if (nxt < 0) {
            nxt = pipe.get_full();
            if (nxt >= 0) upload(o, nxt);
        }
    }
};

// Behind the last chunk: sort and unique on the device (not with -l), the result into `codes` (-T: and taxids_out).
// t0, t1: when the pipeline began and ended, for the --verbose lines.
static u64 finish_count(Windows &w, double t0, double t1, vector<u64> &codes, vector<u32> *taxids_out) {
    Gpu &g = w.g;
    const u64 n = w.n;
    u32 *tax = w.job.tax_re ? w.tax.as<u32>() : nullptr;
    codes.clear();
    u64 nout = n;
    if (!w.job.linear && n) {
        float ms_sort = 0, ms_uniq = 0;
        sort_records(g, w.codes.as<u64>(), tax, n, w.job.key_bits);
        ukm_last_call_ms(g.c, &ms_sort);
        const double t1b = now_ms();
        DevMem dout(g.c, n * 8);
        DevMem dtout(g.c, tax ? n * 4 : 8);
        const double t1c = now_ms();
        ck(ukm_unique(g.c, w.codes.as<u64>(), tax, n, w.job.uniq_mode, (u64 *)dout.p, tax ? (u32 *)dtout.p : nullptr, n, &nout));
        ukm_last_call_ms(g.c, &ms_uniq);
        if (tax && taxids_out) {
            taxids_out->resize(nout ? nout : 1);
            ck(ukm_copy(g.c, taxids_out->data(), dtout.p, nout * 4));
            taxids_out->resize(nout);
        }
        const double t2 = now_ms();
        info("  sort: %.2f ms wall (%.2f ms on the device), output allocation %.2f ms, unique: %.2f ms wall (%.2f ms on the device)",
             t1b - t1, ms_sort, t1c - t1b, t2 - t1c, ms_uniq);
        codes.resize(nout ? nout : 1);
        ck(ukm_copy(g.c, codes.data(), dout.p, nout * 8));
        info("device pipeline: %llu bases in %llu chunk(s); parse+upload+encode %.2f ms (overlapped), sort+unique %.2f ms, download of %llu codes %.2f ms",
             (unsigned long long)w.total_bases, (unsigned long long)w.nchunks, t1 - t0, t2 - t1, (unsigned long long)nout, now_ms() - t2);
    } else {
        codes.resize(n ? n : 1);
        if (n) ck(ukm_copy(g.c, codes.data(), w.codes.p, n * 8));
        if (tax && taxids_out) {
            taxids_out->resize(n ? n : 1);
            if (n) ck(ukm_copy(g.c, taxids_out->data(), tax, n * 4));
            taxids_out->resize(n);
        }
        info("device pipeline: %llu bases in %llu chunk(s); parse+upload+encode %.2f ms (overlapped), download of %llu codes %.2f ms",
             (unsigned long long)w.total_bases, (unsigned long long)w.nchunks, t1 - t0, (unsigned long long)n, now_ms() - t1);
    }
    codes.resize(nout);
    return nout;
}

// Reader, loop and finish wired together.  The result comes back in `codes` (-T: and taxids_out).  Whatever way this is
// left, the destructors run last to first: the stage's device buffers, the reader thread (joined), the page-locked chunks,
// the reader's context, the window arrays -- and the command's context after the call.
static u64 count_on_device(Gpu &g, int device, const CountJob &job, const vector<string> &files, vector<u64> &codes, vector<u32> *taxids_out) {
    // where the bytes are parsed: on the device (ukm_fastx) when asked for, except where a name per record is needed
    const char *host_reason = !job.device_fastx ? "not asked for" : job.skip_name ? "-B" : job.tax_re ? "-T" : nullptr;
    const double t0 = now_ms();
    Windows w(g, job);
    Gpu gp(device);  // the reader thread's own context (page-locked allocations only)
    ChunkPipe pipe({pinned_alloc, pinned_free, gp.c}, job.chunk_bytes + (1 << 20));
    ReaderThread reader(pipe, [&]() {
        if (!host_reason) read_raw_chunks(pipe, files, job.chunk_bytes);
        else read_parsed_chunks(pipe, files, job.chunk_bytes, {job.skip_name, job.tax_re, job.k, job.circular}, job.fastx_report ? host_reason : nullptr);
    });
    if (!host_reason) {
        RawStage stage(w, pipe, files);
        run_double_buffered(pipe, stage);
    } else {
        ParsedStage stage(w, pipe);
        run_double_buffered(pipe, stage);
    }
    reader.join();
    ck(ukm_copy_sync(g.c));
    const string error = pipe.error();
    if (!error.empty()) die("%s", error.c_str());
    return finish_count(w, t0, now_ms(), codes, taxids_out);
}

static int cmd_count(int argc, char **argv) {
    Args a = parse_args(argc, argv, {{'o', "out-prefix", true}, {'k', "kmer-len", true}, {'K', "canonical", false},
                                     {'s', "sort", false}, {'t', "taxid", true}, {'T', "parse-taxid", false},
                                     {'r', "parse-taxid-regexp", true}, {'d', "repeated", false}, {'u', "unique", false},
                                     {'V', "more-verbose", false}, {'H', "hash", false}, {0, "circular", false},
                                     {'D', "scale", true}, {'W', "minimizer-w", true}, {'S', "syncmer-s", true},
                                     {'l', "linear", false}, {'B', "seq-name-filter", true}});
    Options o = get_options(a);
    vector<string> files = get_files(a, o);
    const int k = (int)a.num("kmer-len", 0);
    if (k <= 0) die("value of flag -k/--kmer-len should be positive");
    const bool canonical = a.has("canonical"), sortk = a.has("sort"), linear = a.has("linear");
    bool hashed = a.has("hash");
    const bool repeated = a.has("repeated"), unique = a.has("unique"), circular = a.has("circular");
    if (k > 32 && !hashed) { hashed = true; fprintf(stderr, "[WARN] flag -H/--hash is switched on for k > 32\n"); }  // count.go:81-84
    if (hashed && k > 64) die("k-mer size (%d) should be <=64", k);
    const long long scale = a.num("scale", 1);
    if (scale < 1 || scale > 0x7fffffffLL) die("value of flag --scale is too big");
    const bool scaled = scale > 1;
    if (scaled && !hashed) { hashed = true; fprintf(stderr, "[WARN] flag -H/--hash is switched on for scale > 1\n"); }
    const long long minimizer_w = a.num("minimizer-w", 0);
    if (minimizer_w < 0 || minimizer_w > 0x7fffffffLL) die("value of flag --minimizer-w is too big");
    const bool minimizer = minimizer_w > 0;
    if (minimizer) {  // count.go:100-113 (the sketch itself is always canonical; the -K file flag stays as given)
        if (!hashed) { hashed = true; fprintf(stderr, "[WARN] flag -H/--hash is switched on for minimizer-w > 1\n"); }
        if (!canonical) fprintf(stderr, "[WARN] flag -K/--canonical is switched on for minimizer-w > 1\n");
        if (k > 64) die("k-mer size (%d) should be <=64", k);
    }
    if (a.num("syncmer-s", 0) > 0) die("-S/--syncmer-s is not supported in this build");
    if (repeated && unique) die("flag -d/--repeated and -u/--unique are not compatible");
    const u32 gtaxid = (u32)a.num("taxid", 0);
    const bool parse_taxid = a.has("parse-taxid");
    if (parse_taxid && !a.has("parse-taxid-regexp")) die("flag -r/--parse-taxid-regexp needed when given flag -T/--parse-taxid");
    if (parse_taxid && gtaxid) die("flag -t/--taxid and -T/--parse-taxid can not given simultaneously");
    if (linear && (repeated || unique || sortk)) die("flag -l/--linear is not compatible with -s, -u and -d");
    const string out_file = out_name(a.str("out-prefix", "-"));

    // every mode goes through the device pipeline (round 3: also -T and -W): the parser thread fills page-locked
    // chunks -- with -T it also parses each record's taxid and expands it to the record's windows --, the device thread
    // uploads chunk i + 1 while chunk i is encoded / hashed / sketched, and sort + dedup run on the device
    if (parse_taxid && (scaled || minimizer)) die("-T/--parse-taxid together with -D/--scale or -W/--minimizer-w is not supported in this build");
    Gpu g(o.gpu);
    u32 max_taxid = o.max_taxid;
    if (parse_taxid) max_taxid = load_taxonomy(g, o);
    const u64 max_hash = scaled ? ukm_max_hash((u64)scale) : 0;
    // Scaled sketch: every kept hash is <= maxHash, so the radix sort needs only its significant bits
    // (scale 1000: 55 bits = 7 passes instead of 8)
    int key_bits = hashed ? 64 : 2 * k;
    if (hashed && max_hash != 0) { key_bits = 1; while (key_bits < 64 && (max_hash >> key_bits) != 0) key_bits++; }
    const int uniq_mode = unique ? UKM_SINGLETON : (repeated ? UKM_REPEATED : UKM_UNIQUE);  // count.go:424-436
    vector<u64> codes;
    vector<u32> taxids;
    std::regex re_skip, re_tax;
    if (a.has("seq-name-filter")) re_skip = std::regex(a.str("seq-name-filter"), std::regex::icase);
    if (parse_taxid) re_tax = std::regex(a.str("parse-taxid-regexp"));
    CountJob job;
    job.k = k;
    job.canonical = canonical;
    job.circular = circular;
    job.hashed = hashed;
    job.max_hash = max_hash;
    job.minimizer_w = minimizer ? (int)minimizer_w : 0;
    job.linear = linear;
    job.uniq_mode = uniq_mode;
    job.key_bits = key_bits;
    job.skip_name = a.has("seq-name-filter") ? &re_skip : nullptr;
    job.tax_re = parse_taxid ? &re_tax : nullptr;
    job.device_fastx = o.device_fastx;
    job.fastx_report = o.fastx_report;
    job.chunk_bytes = o.chunk_bytes;
    const u64 n = count_on_device(g, o.gpu, job, files, codes, &taxids);
    u32 mode = 0;
    if (canonical) mode |= unik::UnikCanonical;
    if (parse_taxid) mode |= unik::UnikIncludeTaxID;
    if (hashed) mode |= unik::UnikHashed;
    unik::Header sh;
    if (scaled) { sh.flag |= unik::UnikScaled; sh.scale = (u32)scale; sh.max_hash = max_hash; }
    // without -s the reference writes Go-map order; any order is valid there, we keep the
    // sorted order but only set the Sorted flag (and its encoding) when -s is given
    if (!linear && sortk) mode |= unik::UnikSorted;
    else if (o.compact && !hashed) mode |= unik::UnikCompact;
    write_unik(out_file, o, k, mode, max_taxid, gtaxid, scaled ? &sh : nullptr, codes.data(), taxids.data(), n);
    return 0;
}
