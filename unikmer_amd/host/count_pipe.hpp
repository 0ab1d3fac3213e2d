// count_pipe.hpp — device-free: how the chunks of `count` move between its two threads.  The staging chunk, the pipe the
// reader thread and the device thread share (three chunks go round; the handover of a file to the host parser is ONE
// operation of it), the two reader bodies, the sinks that cut parsed records into chunks, and THE double-buffered loop.
// Like base.hpp and seqtext.hpp it includes nothing of the library: page-locked memory comes through a ChunkAlloc, the
// device work through a stage the loop is handed (cmd_count.hpp).  tests/count_pipe_units.cpp runs it with malloc / free
// under the address, undefined-behaviour and thread sanitizers.
#pragma once
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <regex>
#include <thread>

#include "seqtext.hpp"

// where a chunk's buffer comes from: the driver's is page-locked memory of the reader's context
struct ChunkAlloc {
    void *(*alloc)(void *cookie, u64 bytes);
    void (*free)(void *cookie, void *p);
    void *cookie;
};
// One staging chunk: bases + record boundaries (relative to the chunk).
struct HostChunk {
    ChunkAlloc mem{};
    uint8_t *bases = nullptr;
    u64 cap = 0, nb = 0;
    vector<u64> off{0};
    vector<u32> wtax;  // -T: the taxid of every window of the chunk, in window order (count.go:334-344)
    // the raw reader's chunks (read_raw_chunks): `bases` holds nb raw bytes of input file `file`
    int file = 0;
    bool first = false, last = false, fastq = false;  // the file's first / last chunk; its format, by parse_fastx's rule
    HostChunk() {}
    HostChunk(const HostChunk &) = delete;
    ~HostChunk() { if (bases) mem.free(mem.cookie, bases); }
    void reserve(u64 want) {  // grows the buffer (a record longer than a chunk)
        if (want <= cap) return;
        const u64 ncap = std::max<u64>(want, cap + cap / 2);
        uint8_t *p = (uint8_t *)mem.alloc(mem.cookie, ncap);
        if (nb) memcpy(p, bases, nb);
        if (bases) mem.free(mem.cookie, bases);
        bases = p;
        cap = ncap;
    }
    void reset() { nb = 0; off.assign(1, 0); wtax.clear(); }
};

// reader thread -> device thread hand-off: three chunks go round (one being filled, one travelling, one in the kernels).
// A chunk is named by its index; chunk(i) is touched only by the thread that holds i.
class ChunkPipe {
  public:
    ChunkPipe(const ChunkAlloc &mem, u64 reserve_bytes) {
        for (int i = 0; i < 3; i++) { ch_[i].mem = mem; ch_[i].reserve(reserve_bytes); free_.push_back(i); }
    }
    HostChunk &chunk(int i) { return ch_[i]; }
    // ---- the reader thread's calls
    int get_free() {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return !free_.empty() || abandoned_; });
        if (abandoned_) throw std::runtime_error("count: the chunk pipeline was abandoned");
        return pop(free_);
    }
    void put_full(int i) { { std::lock_guard<std::mutex> l(mu_); full_.push_back(i); } cv_.notify_all(); }
    void finish() { { std::lock_guard<std::mutex> l(mu_); done_ = true; } cv_.notify_all(); }
    void set_error(const string &what) { std::lock_guard<std::mutex> l(mu_); error_ = what; }
    // In front of every read of `file`: when the device thread has asked for the rest of that file, the reader parks -- it
    // reads no more and leaves `in` to the device thread -- until release_reader().  true: the file is no longer the reader's.
    bool park_if_asked(int file, unik::InStream *in) {
        std::unique_lock<std::mutex> l(mu_);
        if (handover_file_ != file) return false;
        stream_ = in; parked_ = true;
        cv_.notify_all();
        cv_.wait(l, [&] { return resume_ || abandoned_; });
        resume_ = parked_ = false; stream_ = nullptr;
        return true;
    }
    // ---- the device thread's calls
    // the next full chunk; -1 once the reader has finished and nothing is queued
    int get_full() {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return !full_.empty() || done_; });
        return full_.empty() ? -1 : pop(full_);
    }
    void put_free(int i) { { std::lock_guard<std::mutex> l(mu_); free_.push_back(i); } cv_.notify_all(); }
    string error() { std::lock_guard<std::mutex> l(mu_); return error_; }
    // The handover: everything of `file` behind the chunk the device thread is at.  Asks the reader to park, takes over the
    // chunk already fetched (nxt, -1: none) and the queued chunks of the file -- up to its last chunk, or until the reader is
    // parked (or done) and nothing is queued -- and gives them back to the free list.  The chunks' bytes in order; whether
    // they end the file; if not, the stream to read on from (the parked reader's; null where the reader died) -- it is the
    // caller's until release_reader().
    struct Rest {
        vector<char> bytes;
        bool exhausted = false;
        unik::InStream *stream = nullptr;
        u64 chunks = 0;
    };
    Rest take_rest_of(int file, int nxt) {
        Rest r;
        std::unique_lock<std::mutex> l(mu_);
        handover_file_ = file;
        for (int i = nxt; !r.exhausted; i = -1) {
            if (i < 0) {
                cv_.wait(l, [&] { return !full_.empty() || parked_ || done_; });
                if (full_.empty()) break;
                i = pop(full_);
            }
            const HostChunk &x = ch_[i];
            r.bytes.insert(r.bytes.end(), (const char *)x.bases, (const char *)x.bases + x.nb);
            r.exhausted = x.last;
            r.chunks++;
            free_.push_back(i);
            cv_.notify_all();  // (the reader may be waiting for this very chunk: the wait below would never end without it)
        }
        if (!r.exhausted) r.stream = stream_;
        return r;
    }
    void release_reader() { { std::lock_guard<std::mutex> l(mu_); if (parked_) resume_ = true; } cv_.notify_all(); }
    // the device thread gives up (an exception on its way out): a reader that waits, now or later, ends with an error
    void abandon() { { std::lock_guard<std::mutex> l(mu_); abandoned_ = true; } cv_.notify_all(); }
    // nothing queued, and each of the three chunks in the free list once: where every run ends
    bool idle() {
        std::lock_guard<std::mutex> l(mu_);
        std::deque<int> f = free_;
        std::sort(f.begin(), f.end());
        return full_.empty() && f == std::deque<int>{0, 1, 2};
    }

  private:
    static int pop(std::deque<int> &q) { const int i = q.front(); q.pop_front(); return i; }
    HostChunk ch_[3];
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<int> full_, free_;
    bool done_ = false, abandoned_ = false;
    string error_;
    int handover_file_ = -1;
    bool parked_ = false, resume_ = false;
    unik::InStream *stream_ = nullptr;
};

// The reader thread around its body.  die() throws there instead of exiting under the device thread's HIP calls: the message
// goes to the pipe's error slot, and the pipe is finished either way.  The destructor joins; a thread that is still running
// then (the device thread is leaving by exception) is woken by abandon().
struct ReaderThread {
    ChunkPipe &pipe;
    std::thread t;
    template <class Body>
    ReaderThread(ChunkPipe &p, Body body) : pipe(p), t([&p, body]() {
        t_worker_thread = true;
        try { body(); } catch (const std::exception &e) { p.set_error(e.what()); }
        p.finish();
    }) {}
    void join() { t.join(); }
    ~ReaderThread() { if (t.joinable()) { pipe.abandon(); t.join(); } }
};

// ---- the reader bodies ------------------------------------------------------------------------------------------------
// The raw reader looks at no byte but the file's first: raw (inflated) bytes, chunk_bytes to a chunk; a file's last chunk is
// its first short read (a file of exactly one chunk: a full chunk, then an empty last one).  before_read, where given, runs in
// front of every read (the unit tests slow the reader down with it).
static void read_raw_chunks(ChunkPipe &pipe, const vector<string> &files, u64 chunk_bytes, void (*before_read)() = nullptr) {
    for (int fi = 0; fi < (int)files.size(); fi++) {
        info("reading sequence file: %s", files[fi].c_str());
        unik::InStream in(files[fi]);
        bool first = true, fastq = false;
        for (;;) {
            if (before_read) before_read();
            if (pipe.park_if_asked(fi, &in)) break;
            const int i = pipe.get_free();
            HostChunk &h = pipe.chunk(i);
            h.reset();
            h.nb = in.read(h.bases, chunk_bytes);
            if (first) fastq = h.nb > 0 && h.bases[0] == '@';
            h.file = fi; h.first = first; h.last = h.nb < chunk_bytes; h.fastq = fastq;
            first = false;
            const bool last = h.last;
            pipe.put_full(i);
            if (last) break;
        }
    }
}

// what the parsing reader does with a record besides its bases
struct RecordRules {
    const std::regex *skip_name = nullptr;  // -B: records whose name matches are left out (count.go:300-312)
    // -T: the taxid is parsed from the header when the record ENDS, and only if the record is long enough to have a
    // window (count.go:323-344: ErrShortSeq is hit before the header is looked at); every window gets its record's taxid
    const std::regex *tax_re = nullptr;
    int k = 0;
    bool circular = false;
};
// parsed records into chunks: a chunk is handed on at the first record end at or behind chunk_bytes
struct ChunkSink : FastxSink {
    ChunkPipe &pipe;
    u64 chunk_bytes;
    RecordRules r;
    int cur;
    string cur_name;
    u64 rec_start = 0;
    ChunkSink(ChunkPipe &p, u64 cb, const RecordRules &rules) : pipe(p), chunk_bytes(cb), r(rules) { cur = pipe.get_free(); pipe.chunk(cur).reset(); }
    bool begin_record(const string &name) override {
        if (r.skip_name && std::regex_search(name, *r.skip_name)) return false;
        if (r.tax_re) cur_name = name;
        rec_start = pipe.chunk(cur).nb;
        return true;
    }
    void add_seq(const char *p, size_t n) override {
        HostChunk &h = pipe.chunk(cur);
        h.reserve(h.nb + n);
        memcpy(h.bases + h.nb, p, n);
        h.nb += n;
    }
    void end_record() override {
        HostChunk &h = pipe.chunk(cur);
        h.off.push_back(h.nb);
        if (r.tax_re) {
            const u64 len = h.nb - rec_start;
            if (len >= (u64)r.k) {
                std::smatch m;
                if (!std::regex_search(cur_name, m, *r.tax_re) || m.size() < 2) die("failed to parse taxid in header: %s", cur_name.c_str());
                const u32 t = (u32)strtoul(m[1].str().c_str(), nullptr, 10);
                h.wtax.insert(h.wtax.end(), r.circular ? len : len - (u64)r.k + 1, t);
            }
        }
        if (h.nb >= chunk_bytes) flush();
    }
    void flush() {
        if (pipe.chunk(cur).off.size() > 1) { pipe.put_full(cur); cur = pipe.get_free(); pipe.chunk(cur).reset(); }
    }
};
// The parsing reader: parse_fastx over every file into record-aligned chunks.  report_reason, where given, is said once
// per file (UNIKMER_FASTX_REPORT: why the host parser has the file).
static void read_parsed_chunks(ChunkPipe &pipe, const vector<string> &files, u64 chunk_bytes, const RecordRules &rules, const char *report_reason) {
    ChunkSink sink(pipe, chunk_bytes, rules);
    for (auto &f : files) {
        info("reading sequence file: %s", f.c_str());
        if (report_reason) fprintf(stderr, "fastx: %s: host (%s)\n", f.c_str(), report_reason);
        parse_fastx(f, sink);
    }
    sink.flush();
}
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

// ---- the double-buffered loop -------------------------------------------------------------------------------------------
// Chunk i+1 travels while chunk i is computed.  The stage has two slots, 0 and 1, and
//   upload(slot, chunk)        starts the chunk's upload into the slot
//   fence()                    the compute calls that follow start behind the uploads started so far
//   compute(slot, other, nxt)  the slot's chunk through the kernels; it gives the chunk back to the pipe.  nxt is the chunk
//                              already on its way to `other` (-1: none); a stage that takes it over puts another in its place.
template <class Stage>
static void run_double_buffered(ChunkPipe &pipe, Stage &stage) {
    int cur = 0;
    int hi = pipe.get_full();
    if (hi >= 0) stage.upload(cur, hi);
    while (hi >= 0) {
        stage.fence();              // kernels of the current chunk start after its upload
        int nxt = pipe.get_full();  // (blocks while the reader is still filling it)
        if (nxt >= 0) stage.upload(cur ^ 1, nxt);
        stage.compute(cur, cur ^ 1, nxt);
        cur ^= 1;
        hi = nxt;
    }
}
