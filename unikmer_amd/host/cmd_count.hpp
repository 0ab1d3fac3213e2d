// cmd_count.hpp — `count` and its chunk pipeline (count.go:41-602)
#pragma once
#include <condition_variable>
#include <ctime>
#include <deque>
#include <functional>
#include <mutex>
#include <regex>
#include <thread>

#include "records.hpp"

// ---- count: device-resident pipeline ------------------------------------------------------------------------
// FASTA/Q bases go to the GPU in record-aligned chunks through two page-locked staging buffers: chunk i+1 is
// uploaded on the context's transfer stream while chunk i is encoded / hashed (count.go:285-299 reads record
// by record; here a "record batch" is a chunk).  The window values never come back to the host: they are
// written to ONE device array, sorted and reduced there (count.go:424-436, 571-581), and only the final set
// crosses PCIe.  Returns the result in `codes`.
static double now_ms() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
// One staging chunk: page-locked bases + record boundaries (relative to the chunk).
struct HostChunk {
    ukm_ctx *c = nullptr;
    uint8_t *bases = nullptr;
    u64 cap = 0, nb = 0;
    vector<u64> off{0};
    vector<u32> wtax;  // -T: the taxid of every window of the chunk, in window order (count.go:334-344)
    // the device parser's chunks (count_on_device, device_fastx): `bases` holds nb raw bytes of input file `file`
    int file = 0;
    bool first = false, last = false, fastq = false;  // the file's first / last chunk; its format, by parse_fastx's rule
    void reserve(u64 want) {  // grows the page-locked buffer (a record longer than a chunk)
        if (want <= cap) return;
        u64 ncap = std::max<u64>(want, cap + cap / 2);
        void *p = nullptr;
        ck(ukm_host_alloc(c, ncap, &p));
        if (nb) memcpy(p, bases, nb);
        if (bases) ukm_host_free(c, bases);
        bases = (uint8_t *)p;
        cap = ncap;
    }
    void reset() { nb = 0; off.assign(1, 0); wtax.clear(); }
};
// parser thread -> device thread hand-off: three chunks go round (one being filled, one travelling, one in the kernels)
struct ChunkPipe {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<int> full, free_;
    bool done = false;
    string error;
    int get_free() { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return !free_.empty(); }); int i = free_.front(); free_.pop_front(); return i; }
    void put_full(int i) { { std::lock_guard<std::mutex> l(mu); full.push_back(i); } cv.notify_all(); }
    int get_full() { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return !full.empty() || done; }); if (full.empty()) return -1; int i = full.front(); full.pop_front(); return i; }
    void put_free(int i) { { std::lock_guard<std::mutex> l(mu); free_.push_back(i); } cv.notify_all(); }
    void finish() { { std::lock_guard<std::mutex> l(mu); done = true; } cv.notify_all(); }
    // The device parser met something outside its grammar in file `handover_file`: the reader thread, if it is still inside
    // that file, parks (it reads no more and leaves `stream`) until the device thread has run the host parser over the rest.
    int handover_file = -1;
    bool parked = false, resume = false;
    unik::InStream *stream = nullptr;
    bool park_if_asked(int file, unik::InStream *in) {  // reader thread, in front of every read
        std::unique_lock<std::mutex> l(mu);
        if (handover_file != file) return false;
        stream = in; parked = true;
        cv.notify_all();
        cv.wait(l, [&] { return resume; });
        resume = parked = false; stream = nullptr;
        return true;
    }
    void ask_handover(int file) { std::lock_guard<std::mutex> l(mu); handover_file = file; }
    // the next full chunk, or -1 once the reader is parked (or done) and nothing is queued
    int get_full_or_parked() { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return !full.empty() || parked || done; }); if (full.empty()) return -1; int i = full.front(); full.pop_front(); return i; }
    void release_reader() { { std::lock_guard<std::mutex> l(mu); if (parked) resume = true; } cv.notify_all(); }
};
// what the host parser gives behind a handover: batches of records, flushed through `out` when they reach a chunk's size
struct BatchFlushSink : FastxSink {
    vector<uint8_t> bases;
    vector<u64> off{0};
    u64 chunk_bytes;
    std::function<void(const uint8_t *, const u64 *, u64, u64)> out;  // (bases, off, records, bytes)
    bool begin_record(const string &) override { return true; }
    void add_seq(const char *p, size_t n) override { bases.insert(bases.end(), p, p + n); }
    void end_record() override { off.push_back(bases.size()); if (bases.size() >= chunk_bytes) flush(); }
    void flush() {
        if (off.size() > 1) out(bases.data(), off.data(), off.size() - 1, bases.size());
        bases.clear(); off.assign(1, 0);
    }
};
struct ChunkSink : FastxSink {
    ChunkPipe &pipe;
    HostChunk *ch;
    u64 chunk_bytes;
    int cur;
    const std::regex *skip_name;
    // -T: the taxid is parsed from the header when the record ENDS, and only if the record is long enough to have a
    // window (count.go:323-344: ErrShortSeq is hit before the header is looked at); every window gets its record's taxid
    const std::regex *tax_re;
    int k;
    bool circular;
    string cur_name;
    u64 rec_start = 0;
    ChunkSink(ChunkPipe &p, HostChunk *c, u64 cb, const std::regex *skip, const std::regex *tre = nullptr, int kk = 0, bool circ = false)
        : pipe(p), ch(c), chunk_bytes(cb), skip_name(skip), tax_re(tre), k(kk), circular(circ) { cur = pipe.get_free(); ch[cur].reset(); }
    bool begin_record(const string &name) override {
        if (skip_name && std::regex_search(name, *skip_name)) return false;  // -B (count.go:300-312)
        if (tax_re) cur_name = name;
        rec_start = ch[cur].nb;
        return true;
    }
    void add_seq(const char *p, size_t n) override {
        HostChunk &h = ch[cur];
        h.reserve(h.nb + n);
        memcpy(h.bases + h.nb, p, n);
        h.nb += n;
    }
    void end_record() override {
        HostChunk &h = ch[cur];
        h.off.push_back(h.nb);
        if (tax_re) {
            const u64 len = h.nb - rec_start;
            if (len >= (u64)k) {
                std::smatch m;
                if (!std::regex_search(cur_name, m, *tax_re) || m.size() < 2) die("failed to parse taxid in header: %s", cur_name.c_str());
                const u32 t = (u32)strtoul(m[1].str().c_str(), nullptr, 10);
                h.wtax.insert(h.wtax.end(), circular ? len : len - (u64)k + 1, t);
            }
        }
        if (h.nb >= chunk_bytes) flush();
    }
    void flush() {
        if (ch[cur].off.size() > 1) { pipe.put_full(cur); cur = pipe.get_free(); ch[cur].reset(); }
    }
};

// device array that grows (the number of windows is unknown while the file is still being read)
struct DevArray {
    ukm_ctx *c;
    u64 *p = nullptr;
    u64 cap = 0;
    explicit DevArray(ukm_ctx *ctx) : c(ctx) {}
    ~DevArray() { if (p) ukm_dev_free(c, p); }
    void ensure(u64 used, u64 want) {
        if (want <= cap) return;
        const u64 ncap = std::max<u64>(want, cap * 2);
        void *q = nullptr;
        ck(ukm_dev_alloc(c, ncap * 8, &q));
        if (used) ck(ukm_copy(c, q, p, used * 8));
        if (p) ukm_dev_free(c, p);
        p = (u64 *)q;
        cap = ncap;
    }
};

static u64 count_on_device(Gpu &g, int device, const vector<string> &files, const std::regex *skip_name, int k, bool canonical, bool circular,
                           bool hashed, u64 max_hash, bool linear, int uniq_mode, int key_bits, vector<u64> &codes,
                           int minimizer_w = 0, const std::regex *tax_re = nullptr, vector<u32> *taxids_out = nullptr,
                           bool device_fastx = false, bool fastx_report = false) {
    // where the bytes are parsed: on the device (ukm_fastx) when asked for, except where a name per record is needed
    const char *host_reason = !device_fastx ? "not asked for" : skip_name ? "-B" : tax_re ? "-T" : nullptr;
    const bool raw = host_reason == nullptr;
    const char *ce = getenv("UNIKMER_CHUNK_MB");
    const u64 CH = (u64)(ce ? std::max(1, atoi(ce)) : 32) << 20;
    const double t0 = now_ms();
    Gpu gp(device);  // the parser thread's own context (page-locked allocations only)
    HostChunk ch[3];
    ChunkPipe pipe;
    for (int i = 0; i < 3; i++) { ch[i].c = gp.c; ch[i].reserve(CH + (1 << 20)); pipe.free_.push_back(i); }
    std::thread parser([&]() {
        t_worker_thread = true;  // die() throws here instead of exiting under the main thread's HIP calls
        try {
            if (raw) {  // the reader looks at no byte but the file's first: raw (inflated) bytes, CH to a chunk
                for (int fi = 0; fi < (int)files.size(); fi++) {
                    info("reading sequence file: %s", files[fi].c_str());
                    unik::InStream in(files[fi]);
                    bool first = true, fastq = false;
                    for (;;) {
                        if (pipe.park_if_asked(fi, &in)) break;
                        const int i = pipe.get_free();
                        HostChunk &h = ch[i];
                        h.reset();
                        h.nb = in.read(h.bases, CH);
                        if (first) fastq = h.nb > 0 && h.bases[0] == '@';
                        h.file = fi; h.first = first; h.last = h.nb < CH; h.fastq = fastq;
                        first = false;
                        const bool last = h.last;
                        pipe.put_full(i);
                        if (last) break;
                    }
                }
                pipe.finish();
                return;
            }
            ChunkSink sink(pipe, ch, CH, skip_name, tax_re, k, circular);
            for (auto &f : files) {
                info("reading sequence file: %s", f.c_str());
                if (fastx_report) fprintf(stderr, "fastx: %s: host (%s)\n", f.c_str(), host_reason);
                parse_fastx(f, sink);
            }
            sink.flush();
        } catch (const std::exception &e) {
            std::lock_guard<std::mutex> l(pipe.mu);
            pipe.error = e.what();
        }
        pipe.finish();
    });
    // device side: chunk i+1 travels (transfer stream) while chunk i is encoded / hashed
    struct Slot { void *bases = nullptr; u64 bcap = 0; void *off = nullptr; u64 ocap = 0; void *tax = nullptr; u64 tcap = 0; int host = -1; u64 nrec = 0; };
    Slot sl[2];
    DevArray dcodes(g.c);
    // -T: the windows' taxids travel with their chunk and are appended to a second growing device array (u32, kept in
    // a u64-granular DevArray: capacity counts pairs of taxids)
    DevArray dtax(g.c);
    const bool with_tax = tax_re != nullptr;
    u64 n = 0, total_bases = 0, nchunks = 0;
    auto upload = [&](Slot &d, int hi) {
        HostChunk &h = ch[hi];
        if (h.nb > d.bcap) { if (d.bases) ukm_dev_free(g.c, d.bases); d.bcap = h.nb + h.nb / 8; ck(ukm_dev_alloc(g.c, d.bcap, &d.bases)); }
        const u64 ob = h.off.size() * 8;
        if (ob > d.ocap) { if (d.off) ukm_dev_free(g.c, d.off); d.ocap = ob + ob / 8; ck(ukm_dev_alloc(g.c, d.ocap, &d.off)); }
        ck(ukm_copy_async(g.c, d.bases, h.bases, h.nb));
        ck(ukm_copy_async(g.c, d.off, h.off.data(), ob));   // (pageable source: staged by the runtime)
        if (with_tax && !h.wtax.empty()) {
            const u64 tb = h.wtax.size() * 4;
            if (tb > d.tcap) { if (d.tax) ukm_dev_free(g.c, d.tax); d.tcap = tb + tb / 8; ck(ukm_dev_alloc(g.c, d.tcap, &d.tax)); }
            ck(ukm_copy_async(g.c, d.tax, h.wtax.data(), tb));
        }
        d.host = hi;
        d.nrec = h.off.size() - 1;
        total_bases += h.nb;
        nchunks++;
    };
    auto compute = [&](Slot &d) {
        HostChunk &h = ch[d.host];
        dcodes.ensure(n, n + h.nb);  // windows <= bases
        u64 m = 0;
        if (minimizer_w > 0) ck(ukm_minimizer(g.c, (const uint8_t *)d.bases, (const u64 *)d.off, d.nrec, k, minimizer_w, circular, max_hash, dcodes.p + n, nullptr, dcodes.cap - n, &m));
        else if (hashed) ck(ukm_nthash(g.c, (const uint8_t *)d.bases, (const u64 *)d.off, d.nrec, k, canonical, circular, max_hash, dcodes.p + n, dcodes.cap - n, &m));
        else ck(ukm_encode_kmers(g.c, (const uint8_t *)d.bases, (const u64 *)d.off, d.nrec, k, canonical, circular, dcodes.p + n, dcodes.cap - n, &m));
        if (with_tax) {
            if (m != h.wtax.size()) die("count -T: %llu windows but %zu taxids in a chunk", (unsigned long long)m, h.wtax.size());
            dtax.ensure((n + 1) / 2, (n + m + 1) / 2 + 1);
            if (m) ck(ukm_copy(g.c, (u32 *)dtax.p + n, d.tax, m * 4));  // device to device, ordered behind the upload by the fence above
        }
        n += m;
        pipe.put_free(d.host);  // its upload is complete (the kernels waited for it): the parser may refill it
        d.host = -1;
    };
    // ---- the device parser: a slot holds a chunk's raw bytes behind `pad` bytes of room, into which the bytes the previous
    // call left unconsumed (an incomplete record) are copied device to device: the text of a call is tail + chunk
    struct RawSlot { uint8_t *text = nullptr; u64 pad = 0, cap = 0, nb = 0; int host = -1; };
    RawSlot rs[2];
    DevMem *dbases = nullptr, *drec = nullptr;
    u64 dbases_cap = 0, drec_cap = 0;
    auto encode = [&](const uint8_t *bases, const u64 *off, u64 nrec, u64 nb) {  // host or device pointers
        dcodes.ensure(n, n + nb);  // windows <= bases
        u64 m = 0;
        if (minimizer_w > 0) ck(ukm_minimizer(g.c, bases, off, nrec, k, minimizer_w, circular, max_hash, dcodes.p + n, nullptr, dcodes.cap - n, &m));
        else if (hashed) ck(ukm_nthash(g.c, bases, off, nrec, k, canonical, circular, max_hash, dcodes.p + n, dcodes.cap - n, &m));
        else ck(ukm_encode_kmers(g.c, bases, off, nrec, k, canonical, circular, dcodes.p + n, dcodes.cap - n, &m));
        n += m;
        total_bases += nb;
    };
    auto raw_room = [&](RawSlot &d, u64 pad, u64 data) {  // at least `pad` bytes in front of `data` bytes; keeps the chunk in it
        if (d.text && d.pad >= pad && d.cap - d.pad >= data) return;
        ck(ukm_copy_sync(g.c));  // (an upload into the old buffer may be on its way)
        const u64 npad = d.text ? std::max<u64>((pad + pad / 2 + 15) & ~(u64)15, d.pad) : ((pad + 15) & ~(u64)15);
        const u64 ndata = std::max<u64>(data, d.text ? d.cap - d.pad : 0);
        void *p = nullptr;
        ck(ukm_dev_alloc(g.c, npad + ndata, &p));
        if (d.text) { if (d.nb) ck(ukm_copy(g.c, (uint8_t *)p + npad, d.text + d.pad, d.nb)); ukm_dev_free(g.c, d.text); }
        d.text = (uint8_t *)p; d.pad = npad; d.cap = npad + ndata;
    };
    auto upload_raw = [&](RawSlot &d, int hi) {
        HostChunk &h = ch[hi];
        raw_room(d, 1 << 20, CH);
        d.nb = h.nb;
        if (h.nb) ck(ukm_copy_async(g.c, d.text + d.pad, h.bases, h.nb));
        d.host = hi;
        nchunks++;
    };
    u64 tail = 0, fpos = 0, fchunks = 0;  // unconsumed bytes in front of the current chunk; the file offset they start at
    // chunk d through ukm_fastx and the encode kernels; nxt: the chunk already uploaded to `other` (-1: none), taken over by a handover
    auto compute_raw = [&](RawSlot &d, RawSlot &other, int &nxt) {
        HostChunk &h = ch[d.host];
        const int fi = h.file;
        const bool last = h.last, fastq = h.fastq;
        if (h.first) { fpos = 0; fchunks = 0; }  // (records never span files: the tail is empty)
        fchunks++;
        const uint8_t *text = d.text + d.pad - tail;
        const u64 nt = tail + d.nb;
        u64 nb = 0, nrec = 0, used = 0;
        int stop = UKM_FASTX_STOP_NONE;
        if (nt) {
            // the most a text can hold: every byte a base; a record in two bytes
            const u64 rcap = nt / 2 + 1;
            if (dbases_cap < nt) { delete dbases; dbases_cap = nt + nt / 8; dbases = new DevMem(g.c, dbases_cap); }
            if (drec_cap < rcap) { delete drec; drec_cap = rcap + rcap / 8; drec = new DevMem(g.c, (drec_cap + 1) * 8); }
            ck(ukm_fastx(g.c, text, nt, (fastq ? UKM_FASTX_FASTQ : 0u) | (last ? UKM_FASTX_LAST : 0u), (uint8_t *)dbases->p, dbases_cap,
                         (u64 *)drec->p, nullptr, drec_cap, &nb, &nrec, &used, &stop));
            if (nrec) encode((const uint8_t *)dbases->p, (const u64 *)drec->p, nrec, nb);
        }
        pipe.put_free(d.host);  // its upload is complete (the kernels waited for it): the reader may refill it
        d.host = -1;
        if (stop != UKM_FASTX_STOP_GRAMMAR) {
            tail = nt - used;
            fpos += used;
            if (tail) {  // in front of the next chunk, device to device (a record longer than the room: the room grows)
                raw_room(other, tail, CH);
                ck(ukm_copy(g.c, other.text + other.pad - tail, text + used, tail));
            }
            if (last && fastx_report) fprintf(stderr, "fastx: %s: device, %llu chunk(s)\n", files[fi].c_str(), (unsigned long long)fchunks);
            return;
        }
        // outside the device's grammar: the rest of the file -- what is left of this text, the chunks already read, the stream --
        // goes through the host parser, from a byte at which its state machine expects a header
        vector<char> mem(nt - used);
        if (!mem.empty()) ck(ukm_copy(g.c, mem.data(), text + used, mem.size()));
        tail = 0;
        bool exhausted = last;
        if (!exhausted) {
            pipe.ask_handover(fi);
            auto take = [&](int i) {
                HostChunk &x = ch[i];
                mem.insert(mem.end(), (const char *)x.bases, (const char *)x.bases + x.nb);
                exhausted = x.last;
                fchunks++;
                pipe.put_free(i);
            };
            if (nxt >= 0) { ck(ukm_copy_sync(g.c)); other.host = -1; other.nb = 0; take(nxt); nxt = -1; }
            while (!exhausted) {
                const int i = pipe.get_full_or_parked();
                if (i < 0) break;
                nchunks++;
                take(i);
            }
        }
        BatchFlushSink sink;
        sink.chunk_bytes = CH;
        sink.out = encode;
        parse_fastx(mem.data(), mem.size(), exhausted ? nullptr : pipe.stream, fastq, files[fi], sink);
        sink.flush();
        pipe.release_reader();
        if (fastx_report)
            fprintf(stderr, "fastx: %s: device, %llu chunk(s), host from byte %llu (grammar)\n", files[fi].c_str(), (unsigned long long)fchunks,
                    (unsigned long long)(fpos + used));
        if (nxt < 0) {  // the chunk that was on its way has been taken over: the next file's first
            nxt = pipe.get_full();
            if (nxt >= 0) upload_raw(other, nxt);
        }
    };
    int cur = 0;
    int hi = pipe.get_full();
    if (raw) {
        if (hi >= 0) upload_raw(rs[cur], hi);
        while (hi >= 0) {
            ck(ukm_copy_fence(g.c));    // kernels of the current chunk start after its upload
            int nxt = pipe.get_full();  // (blocks while the reader is still filling it)
            if (nxt >= 0) upload_raw(rs[cur ^ 1], nxt);
            compute_raw(rs[cur], rs[cur ^ 1], nxt);
            cur ^= 1;
            hi = nxt;
        }
        for (auto &d : rs) if (d.text) ukm_dev_free(g.c, d.text);
        delete dbases;
        delete drec;
        hi = -1;
    }
    if (hi >= 0) upload(sl[cur], hi);
    while (hi >= 0) {
        ck(ukm_copy_fence(g.c));            // kernels of the current chunk start after its upload
        const int nxt = pipe.get_full();    // (blocks while the parser is still filling it)
        if (nxt >= 0) upload(sl[cur ^ 1], nxt);
        compute(sl[cur]);
        cur ^= 1;
        hi = nxt;
    }
    parser.join();
    ck(ukm_copy_sync(g.c));
    for (auto &d : sl) { if (d.bases) ukm_dev_free(g.c, d.bases); if (d.off) ukm_dev_free(g.c, d.off); if (d.tax) ukm_dev_free(g.c, d.tax); }
    for (auto &h : ch) if (h.bases) ukm_host_free(gp.c, h.bases);
    if (!pipe.error.empty()) die("%s", pipe.error.c_str());
    const double t1 = now_ms();
    codes.clear();
    u64 nout = n;
    if (!linear && n) {
        float ms_sort = 0, ms_uniq = 0;
        sort_records(g, dcodes.p, with_tax ? (u32 *)dtax.p : nullptr, n, key_bits);
        ukm_last_call_ms(g.c, &ms_sort);
        const double t1b = now_ms();
        DevMem dout(g.c, n * 8);
        DevMem dtout(g.c, with_tax ? n * 4 : 8);
        const double t1c = now_ms();
        ck(ukm_unique(g.c, dcodes.p, with_tax ? (u32 *)dtax.p : nullptr, n, uniq_mode, (u64 *)dout.p, with_tax ? (u32 *)dtout.p : nullptr, n, &nout));
        ukm_last_call_ms(g.c, &ms_uniq);
        if (with_tax && taxids_out) {
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
             (unsigned long long)total_bases, (unsigned long long)nchunks, t1 - t0, t2 - t1, (unsigned long long)nout, now_ms() - t2);
    } else {
        codes.resize(n ? n : 1);
        if (n) ck(ukm_copy(g.c, codes.data(), dcodes.p, n * 8));
        if (with_tax && taxids_out) {
            taxids_out->resize(n ? n : 1);
            if (n) ck(ukm_copy(g.c, taxids_out->data(), dtax.p, n * 4));
            taxids_out->resize(n);
        }
        info("device pipeline: %llu bases in %llu chunk(s); parse+upload+encode %.2f ms (overlapped), download of %llu codes %.2f ms",
             (unsigned long long)total_bases, (unsigned long long)nchunks, t1 - t0, (unsigned long long)n, now_ms() - t1);
    }
    codes.resize(nout);
    return nout;
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
    const u64 n = count_on_device(g, o.gpu, files, a.has("seq-name-filter") ? &re_skip : nullptr, k, canonical, circular, hashed, max_hash, linear,
                                  uniq_mode, key_bits, codes, minimizer ? (int)minimizer_w : 0, parse_taxid ? &re_tax : nullptr, &taxids,
                                  o.device_fastx, o.fastx_report);
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
