// unik.hpp — reader/writer of the `.unik` v5.0 container, the C++ stand-in for
// github.com/shenwei356/unik/v5 v5.0.1 as the reference uses it (unik.NewReader /
// ReadCodeWithTaxid / NewWriter / WriteCode / WriteCodeWithTaxid / WriteTaxid / Flush /
// SetMaxTaxid / SetGlobalTaxid / SetScale / Number; e.g. union.go:136,171,187,251).
//
// PARITY UNPINNED: the reference tree holds neither a `.unik` file nor a format description
// (`.gitignore` excludes *.unik) and the module source is not vendored.  The byte layout
// below is the reconstruction of SURVEY.md Appendix B6; it is self-consistent (everything this
// tool writes it reads back) but has not been checked against a file written by the Go tool.
//
// Layout (big-endian throughout):
//   magic ".unikmer" (8) | main=5, minor=0, K, 0 (4 x u8) | Flag u32 | Number u64
//   | globalTaxid u32 | taxidBytesLen u8 | 3 x 0 | descLen u32 | desc | scale u32 | maxHash u64
//   | 52 reserved zero bytes
//   body, unsorted: per record  code (8 bytes, or (k+3)/4 bytes when Compact) [taxid]
//   body, sorted  : records in pairs: ctrl = ((len0-1)<<3)|(len1-1), then len0 bytes of
//                   (c0 - prev) and len1 bytes of (c1 - c0), prev = c1, [taxid0][taxid1];
//                   a trailing odd record: ctrl = 128, 8 bytes of the full code [taxid]
//   taxid = taxidBytesLen big-endian bytes, present when IncludeTaxID.
// The whole stream is optionally gzip (zlib's gz* API reads plain and gzip transparently,
// like util-io.go:99-101 sniffing 1f 8b).
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace unik {

enum : uint32_t {
    UnikCompact = 1u << 0,
    UnikCanonical = 1u << 1,
    UnikSorted = 1u << 2,
    UnikIncludeTaxID = 1u << 3,
    UnikHashed = 1u << 4,
    UnikScaled = 1u << 5,
};

struct Header {
    uint8_t main_version = 5, minor_version = 0;
    int k = 0;
    uint32_t flag = 0;
    uint64_t number = ~0ull;  // 0xFFFF.. (prints as -1) or 0 = unknown (concat.go:69, info.go:379)
    uint32_t global_taxid = 0;
    uint8_t taxid_bytes = 4;
    std::string description;
    uint32_t scale = 1;
    uint64_t max_hash = ~0ull;

    bool is_compact() const { return flag & UnikCompact; }
    bool is_canonical() const { return flag & UnikCanonical; }
    bool is_sorted() const { return flag & UnikSorted; }
    bool is_include_taxid() const { return flag & UnikIncludeTaxID; }
    bool is_hashed() const { return flag & UnikHashed; }
    bool is_scaled() const { return flag & UnikScaled; }
    bool has_global_taxid() const { return global_taxid > 0; }
    bool has_taxid_info() const { return is_include_taxid() || has_global_taxid(); }
};

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline int taxid_bytes_for(uint32_t max_taxid) {  // util.go:340-342 maxUint32N inverse
    if (max_taxid <= 0xFF) return 1;
    if (max_taxid <= 0xFFFF) return 2;
    if (max_taxid <= 0xFFFFFF) return 3;
    return 4;
}

// ---- byte streams over zlib ---------------------------------------------------------------------
class InStream {
  public:
    explicit InStream(const std::string &path) : path_(path) {
        if (path == "-") gz_ = gzdopen(fileno(stdin), "rb");
        else gz_ = gzopen(path.c_str(), "rb");
        if (!gz_) throw Error("fail to open file: " + path);
        gzbuffer(gz_, 1 << 20);
    }
    ~InStream() { if (gz_) gzclose(gz_); }
    InStream(const InStream &) = delete;
    // returns number of bytes read (< n only at EOF)
    size_t read(void *dst, size_t n) {
        size_t got = 0;
        while (got < n) {
            int r = gzread(gz_, (char *)dst + got, (unsigned)std::min<size_t>(n - got, 1u << 30));
            if (r < 0) throw Error("read error: " + path_);
            if (r == 0) break;
            got += (size_t)r;
        }
        return got;
    }
    void must_read(void *dst, size_t n) {
        if (read(dst, n) != n) throw Error("unexpected EOF: " + path_);
    }
    bool gzipped() const { return !gzdirect(gz_); }
    gzFile raw() { return gz_; }

  private:
    std::string path_;
    gzFile gz_ = nullptr;
};

// Three forms: a plain file; gzip through zlib's gz* API; and "device gzip": a plain file that holds ONE gzip member whose
// deflate stream this class assembles -- small writes (the header, a Writer's trailing bytes) go through a raw zlib deflate
// stream, a body that was deflated elsewhere (ukm_deflate: a byte-aligned run of blocks, none final) is appended as it is
// behind a sync flush, and the CRC-32 runs alongside.  Header, body and trailing bytes may come in any order of calls.
class OutStream {
  public:
    OutStream(const std::string &path, bool compress, int level, bool device_gzip = false) : path_(path) {
        if (compress && device_gzip && level != 0) {
            open_plain();
            memset(&z_, 0, sizeof z_);
            if (deflateInit2(&z_, level < 0 ? 6 : (level > 9 ? 9 : level), Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK)
                throw Error("fail to write file: " + path);
            dz_ = true;
            zbuf_.resize(1 << 16);
            const uint8_t head[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255};  // RFC 1952: no flags, no time, OS unknown
            put_plain(head, sizeof head);
        } else if (compress) {
            std::string mode = "wb" + std::to_string(level < 0 ? 6 : (level > 9 ? 9 : level));
            gz_ = (path == "-") ? gzdopen(fileno(stdout), mode.c_str()) : gzopen(path.c_str(), mode.c_str());
            if (!gz_) throw Error("fail to write file: " + path);
            gzbuffer(gz_, 1 << 20);
        } else {
            open_plain();
        }
    }
    ~OutStream() {
        try { close(); } catch (...) {}
    }
    OutStream(const OutStream &) = delete;
    bool device_gzip() const { return dz_; }
    void write(const void *src, size_t n) {
        if (n == 0) return;
        if (dz_) {
            size_t done = 0;
            while (done < n) {
                const uInt chunk = (uInt)std::min<size_t>(n - done, 1u << 30);
                crc_ = crc32(crc_, (const Bytef *)src + done, chunk);
                z_.next_in = (Bytef *)const_cast<void *>(src) + done;
                z_.avail_in = chunk;
                run_deflate(Z_NO_FLUSH);
                done += chunk;
            }
            raw_len_ += n;
        } else if (gz_) {
            size_t done = 0;
            while (done < n) {
                unsigned chunk = (unsigned)std::min<size_t>(n - done, 1u << 30);
                if (gzwrite(gz_, (const char *)src + done, chunk) != (int)chunk) throw Error("write error: " + path_);
                done += chunk;
            }
        } else {
            put_plain(src, n);
        }
    }
    // device gzip only: `fragment` is raw_len bytes deflated elsewhere as a byte-aligned run of blocks without a final one;
    // crc_of_raw = the CRC-32 of those raw_len bytes alone
    void write_deflated(const void *fragment, size_t n, uint32_t crc_of_raw, uint64_t raw_len) {
        if (!dz_) throw Error("write error: " + path_);
        z_.next_in = nullptr;
        z_.avail_in = 0;
        run_deflate(Z_SYNC_FLUSH);  // ends on a byte boundary
        put_plain(fragment, n);
        static_assert(sizeof(z_off_t) == 8, "bodies are longer than 2 GiB");
        crc_ = (uint32_t)crc32_combine(crc_, crc_of_raw, (z_off_t)raw_len);
        raw_len_ += raw_len;
    }
    void close() {
        if (dz_) {
            dz_ = false;
            z_.next_in = nullptr;
            z_.avail_in = 0;
            run_deflate(Z_FINISH);
            deflateEnd(&z_);
            uint8_t tail[8];
            for (int i = 0; i < 4; i++) {
                tail[i] = (uint8_t)(crc_ >> (8 * i));
                tail[4 + i] = (uint8_t)(raw_len_ >> (8 * i));
            }
            put_plain(tail, sizeof tail);
        }
        if (gz_) { gzclose(gz_); gz_ = nullptr; }
        if (fp_) { if (fp_ != stdout) fclose(fp_); else fflush(fp_); fp_ = nullptr; }
    }

  private:
    void open_plain() {
        fp_ = (path_ == "-") ? stdout : fopen(path_.c_str(), "wb");
        if (!fp_) throw Error("fail to write file: " + path_);
    }
    void put_plain(const void *src, size_t n) {
        if (n && fwrite(src, 1, n, fp_) != n) throw Error("write error: " + path_);
    }
    // everything zlib will give for the input at hand, to the file
    void run_deflate(int flush) {
        for (;;) {
            z_.next_out = zbuf_.data();
            z_.avail_out = (uInt)zbuf_.size();
            const int rc = deflate(&z_, flush);
            if (rc == Z_STREAM_ERROR) throw Error("write error: " + path_);
            put_plain(zbuf_.data(), zbuf_.size() - z_.avail_out);
            if (z_.avail_out != 0) break;  // (Z_BUF_ERROR: nothing was pending, e.g. a second flush in a row)
        }
    }
    std::string path_;
    gzFile gz_ = nullptr;
    FILE *fp_ = nullptr;
    bool dz_ = false;
    z_stream z_;
    std::vector<uint8_t> zbuf_;
    uint32_t crc_ = 0;
    uint64_t raw_len_ = 0;
};

static inline void put_be(uint8_t *p, uint64_t v, int n) {
    for (int i = n - 1; i >= 0; i--) { p[i] = (uint8_t)v; v >>= 8; }
}
static inline uint64_t get_be(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[i];
    return v;
}
static inline int byte_len(uint64_t v) {
    int n = 1;
    while (v >>= 8) n++;
    return n;
}

// The header, from anything that has InStream's read / must_read: the file's stream (Reader), or the header's bytes as zlib
// inflated them (GzInput).  The one statement of the layout on the reading side.
template <class In>
static inline void read_header_from(In &in, Header &h, const std::string &path) {
    uint8_t b[64];
    if (in.read(b, 8) != 8 || memcmp(b, ".unikmer", 8) != 0) throw Error("invalid binary format: " + path);
    in.must_read(b, 4);
    h.main_version = b[0]; h.minor_version = b[1]; h.k = b[2];
    if (h.main_version != 5) throw Error("version mismatch (need v5.x): " + path);
    in.must_read(b, 4); h.flag = (uint32_t)get_be(b, 4);
    in.must_read(b, 8); h.number = get_be(b, 8);
    in.must_read(b, 4); h.global_taxid = (uint32_t)get_be(b, 4);
    in.must_read(b, 4); h.taxid_bytes = b[0];
    if (h.taxid_bytes < 1 || h.taxid_bytes > 4) throw Error("bad taxid byte length: " + path);
    in.must_read(b, 4);
    const uint32_t dl = (uint32_t)get_be(b, 4);
    if (dl > 1024) throw Error("description too long: " + path);
    h.description.resize(dl);
    if (dl) in.must_read(&h.description[0], dl);
    in.must_read(b, 4); h.scale = (uint32_t)get_be(b, 4);
    in.must_read(b, 8); h.max_hash = get_be(b, 8);
    in.must_read(b, 52);
}
struct MemStream {  // bytes in memory behind InStream's two calls
    const uint8_t *p;
    size_t n, at = 0;
    size_t read(void *dst, size_t want) {
        const size_t got = std::min(want, n - at);
        memcpy(dst, p + at, got);
        at += got;
        return got;
    }
    void must_read(void *dst, size_t want) {
        if (read(dst, want) != want) throw Error("unexpected EOF");
    }
};

// ---- Reader -------------------------------------------------------------------------------------
class Reader {
  public:
    Header h;
    explicit Reader(const std::string &path) : in_(path), path_(path) { read_header(); }

    bool gzipped() const { return in_.gzipped(); }

    // unik.Reader.ReadCodeWithTaxid: false at EOF.  When the file has only a global taxid it is
    // returned for every record.
    bool read(uint64_t &code, uint32_t &taxid) {
        taxid = h.global_taxid;
        if (!h.is_sorted()) {
            uint8_t b[8];
            const int n = h.is_compact() ? (h.k + 3) / 4 : 8;
            size_t got = in_.read(b, (size_t)n);
            if (got == 0) return false;
            if (got != (size_t)n) throw Error("truncated record: " + path_);
            code = get_be(b, n);
            if (h.is_include_taxid()) taxid = read_taxid();
            return true;
        }
        if (have_second_) {
            code = second_;
            taxid = h.is_include_taxid() ? second_taxid_ : h.global_taxid;
            have_second_ = false;
            return true;
        }
        uint8_t ctrl;
        if (in_.read(&ctrl, 1) == 0) return false;
        uint8_t b[16];
        if (ctrl & 128) {  // trailing single record: the full code
            in_.must_read(b, 8);
            code = get_be(b, 8);
            prev_ = code;
            if (h.is_include_taxid()) taxid = read_taxid();
            return true;
        }
        const int l0 = ((ctrl >> 3) & 7) + 1, l1 = (ctrl & 7) + 1;
        in_.must_read(b, (size_t)(l0 + l1));
        const uint64_t c0 = prev_ + get_be(b, l0);
        const uint64_t c1 = c0 + get_be(b + l0, l1);
        prev_ = c1;
        code = c0;
        second_ = c1;
        have_second_ = true;
        if (h.is_include_taxid()) {
            taxid = read_taxid();
            second_taxid_ = read_taxid();
        }
        return true;
    }

    // bulk: append every record; taxids filled when the file carries taxid information
    void read_all(std::vector<uint64_t> &codes, std::vector<uint32_t> *taxids) {
        uint64_t c;
        uint32_t t;
        if (h.number != ~0ull && h.number != 0) {
            codes.reserve(codes.size() + h.number);
            if (taxids) taxids->reserve(taxids->size() + h.number);
        }
        while (read(c, t)) {
            codes.push_back(c);
            if (taxids) taxids->push_back(t);
        }
    }

    // bulk: everything behind the header, inflated, as it stands in the file (what ukm_unik_decode takes).  Not to be
    // mixed with read() on one Reader.
    void read_body(std::vector<uint8_t> &body) {
        size_t chunk = 1u << 22;
        for (;;) {
            const size_t at = body.size();
            body.resize(at + chunk);
            const size_t got = in_.read(body.data() + at, chunk);
            body.resize(at + got);
            if (got < chunk) break;
            if (chunk < (1u << 28)) chunk <<= 1;
        }
    }

  private:
    uint32_t read_taxid() {
        uint8_t b[4];
        in_.must_read(b, h.taxid_bytes);
        return (uint32_t)get_be(b, h.taxid_bytes);
    }
    void read_header() { read_header_from(in_, h, path_); }

    InStream in_;
    std::string path_;
    uint64_t prev_ = 0, second_ = 0;
    uint32_t second_taxid_ = 0;
    bool have_second_ = false;
};

// ---- a gzip input whose body is inflated elsewhere ----------------------------------------------------
// The host's part of reading a file that OutStream's device-gzip mode wrote (or Python's save(deflate="device")) without
// zlib inflating the body: open() takes the gzip framing off and lets zlib read the .unik header up to the sync-flush marker
// behind it; the caller hands file[body_at, body_end) to ukm_inflate, which says how far it got; finish() lets zlib read what
// is left behind that point (the final block; a Writer's trailing odd record) with the output so far as its dictionary, and
// checks the trailer.  Both return "" or the reason why the file is to be read through InStream instead: nothing here is an
// error, the host path meets the same bytes and names what is wrong with them.
struct GzInput {
    std::vector<uint8_t> file;
    Header h;
    std::vector<uint8_t> header_bytes;  // the .unik header as it was inflated
    size_t body_at = 0, body_end = 0;   // file[body_at, body_end): the deflate stream behind the header's marker, in front of the trailer
    uint32_t header_crc = 0;            // CRC-32 of header_bytes: what the body's CRC is chained to

    static constexpr size_t HEADER_FIXED = 36, HEADER_TAIL = 64, DESC_MAX = 1024;

    std::string open(const std::string &path) {
        if (path == "-") return "stdin";
        FILE *f = fopen(path.c_str(), "rb");
        if (!f) return "cannot be opened";
        bool ok = fseek(f, 0, SEEK_END) == 0;
        const long size = ok ? ftell(f) : -1;
        ok = ok && size >= 0 && fseek(f, 0, SEEK_SET) == 0;
        if (ok) {
            file.resize((size_t)size);
            ok = fread(file.data(), 1, file.size(), f) == file.size();
        }
        fclose(f);
        if (!ok) return "not a regular file";
        return open_bytes();
    }
    // the same on `file` as it stands
    std::string open_bytes() {
        if (file.size() < 2 || file[0] != 0x1f || file[1] != 0x8b) return "not gzip";
        if (file.size() < 18 || file[2] != 8) return "not a gzip member";
        if (file[3] != 0) return "gzip header with FLG != 0";
        body_end = file.size() - 8;
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) return "inflateInit2";
        header_bytes.assign(HEADER_FIXED + DESC_MAX + HEADER_TAIL + 1, 0);
        z.next_in = file.data() + 10;
        z.avail_in = (uInt)std::min<size_t>(body_end - 10, 1u << 20);
        z.next_out = header_bytes.data();
        z.avail_out = (uInt)header_bytes.size();
        size_t need = 0;
        std::string why;
        for (;;) {
            const int rc = inflate(&z, Z_BLOCK);  // returns at every block boundary
            if (rc != Z_OK) {
                why = rc == Z_STREAM_END ? "the stream ends with the header's block" : std::string("the header: ") + (z.msg ? z.msg : "zlib stops");
                break;
            }
            if (!need && z.total_out >= HEADER_FIXED) {
                const uint64_t dl = get_be_(header_bytes.data() + 32, 4);
                if (dl > DESC_MAX) {
                    why = "description too long";
                    break;
                }
                need = HEADER_FIXED + (size_t)dl + HEADER_TAIL;
            }
            if ((need && z.total_out > need) || z.avail_out == 0) {
                why = "the header does not end at a block boundary";
                break;
            }
            // "a block just ended, not the last one, no unused bits", the header exactly out, and the marker just read
            const bool boundary = (z.data_type & 128) && !(z.data_type & 64) && (z.data_type & 63) == 0;
            if (need && z.total_out == need && boundary && z.total_in >= 4 && memcmp(z.next_in - 4, "\x00\x00\xff\xff", 4) == 0) break;
            if (z.avail_in == 0) {
                why = "the header does not end at a sync flush";
                break;
            }
        }
        body_at = 10 + (size_t)z.total_in;
        inflateEnd(&z);
        if (!why.empty()) return why;
        header_bytes.resize(need);
        header_crc = (uint32_t)crc32(0, header_bytes.data(), (uInt)need);
        return parse_header();
    }
    // the size of the inflated body, the trailing bytes included, from the trailer's ISIZE (the total modulo 2^32): the
    // smallest that n compressed bytes can inflate to -- stored framing takes less than a byte per 4096 -- and 0 where that
    // is above 8 bytes per byte
    uint64_t body_total() const {
        const uint64_t n = body_end - body_at, low = n - std::min<uint64_t>(n, n / 4096 + 64);
        uint64_t total = (uint32_t)(isize() - (uint32_t)header_bytes.size());
        while (total < low) total += 1ull << 32;
        return total > 8 * n ? 0 : total;
    }
    // consumed, n_out, crc: what ukm_inflate gave for file[body_at, body_end) with *crc32 = header_crc on entry; last: the
    // last min(n_out, 32768) bytes of its output.  *tail: the bytes that follow them in the body.
    std::string finish(uint64_t consumed, uint64_t n_out, uint32_t crc, const uint8_t *last, size_t n_last, std::vector<uint8_t> *tail) {
        tail->clear();
        if (consumed > body_end - body_at) return "consumed more than there is";
        std::vector<uint8_t> dict;
        if (n_last < 32768) dict.assign(header_bytes.end() - (std::ptrdiff_t)std::min<size_t>(header_bytes.size(), 32768 - n_last), header_bytes.end());
        dict.insert(dict.end(), last, last + n_last);
        z_stream z;
        memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) return "inflateInit2";
        std::string why;
        if (!dict.empty() && inflateSetDictionary(&z, dict.data(), (uInt)dict.size()) != Z_OK) why = "inflateSetDictionary";
        size_t at = body_at + (size_t)consumed;
        int rc = Z_OK;
        while (why.empty() && rc != Z_STREAM_END) {
            const size_t have = tail->size();
            tail->resize(have + (1u << 16));
            z.next_out = tail->data() + have;
            z.avail_out = 1u << 16;
            z.next_in = file.data() + at;
            z.avail_in = (uInt)std::min<size_t>(body_end - at, 1u << 30);
            const uInt fed = z.avail_in;
            rc = inflate(&z, Z_NO_FLUSH);
            at += fed - z.avail_in;
            tail->resize(have + ((1u << 16) - z.avail_out));
            if (rc == Z_STREAM_END) break;
            if (rc != Z_OK && rc != Z_BUF_ERROR) why = std::string("behind the device's part: ") + (z.msg ? z.msg : "zlib stops");
            else if (at == body_end && z.avail_out != 0) why = "the stream does not end in front of the trailer";
        }
        inflateEnd(&z);
        if (!why.empty()) return why;
        if (at != body_end) return "bytes behind the deflate stream (a second member?)";
        crc = (uint32_t)crc32(crc, tail->data(), (uInt)tail->size());
        if (crc != (uint32_t)get_le_(file.data() + body_end, 4)) return "CRC-32 mismatch";
        if ((uint32_t)(header_bytes.size() + n_out + tail->size()) != isize()) return "size mismatch";
        return "";
    }
    uint32_t isize() const { return (uint32_t)get_le_(file.data() + body_end + 4, 4); }

  private:
    static uint64_t get_be_(const uint8_t *p, int n) {
        uint64_t v = 0;
        for (int i = 0; i < n; i++) v = (v << 8) | p[i];
        return v;
    }
    static uint64_t get_le_(const uint8_t *p, int n) {
        uint64_t v = 0;
        for (int i = n - 1; i >= 0; i--) v = (v << 8) | p[i];
        return v;
    }
    // the Reader's own routine on the inflated bytes; what it refuses goes the host's way and is refused there, with the path
    std::string parse_header() {
        MemStream m{header_bytes.data(), header_bytes.size()};
        try {
            read_header_from(m, h, "");
        } catch (const Error &e) {
            return e.what();
        }
        return m.at == header_bytes.size() ? "" : "the header's size";
    }
};

// ---- Writer -------------------------------------------------------------------------------------
class Writer {
  public:
    Header h;
    Writer(OutStream &out, int k, uint32_t mode) : out_(out) {
        h.k = k;
        h.flag = mode;
        buf_.reserve(1 << 20);
    }
    void set_max_taxid(uint32_t m) { h.taxid_bytes = (uint8_t)taxid_bytes_for(m); }
    void set_global_taxid(uint32_t t) { h.global_taxid = t; }
    void set_scale(uint32_t scale, uint64_t max_hash) {  // count.go:254-256,469-471
        h.scale = scale;
        h.max_hash = max_hash;
        h.flag |= UnikScaled;
    }
    void set_number(uint64_t n) { h.number = n; }

    void write_header() {
        if (wrote_header_) return;
        wrote_header_ = true;
        uint8_t b[64] = {0};
        out_.write(".unikmer", 8);
        b[0] = h.main_version; b[1] = h.minor_version; b[2] = (uint8_t)h.k; b[3] = 0;
        out_.write(b, 4);
        put_be(b, h.flag, 4); out_.write(b, 4);
        put_be(b, h.number, 8); out_.write(b, 8);
        put_be(b, h.global_taxid, 4); out_.write(b, 4);
        b[0] = h.taxid_bytes; b[1] = b[2] = b[3] = 0; out_.write(b, 4);
        put_be(b, h.description.size(), 4); out_.write(b, 4);
        out_.write(h.description.data(), h.description.size());
        put_be(b, h.scale, 4); out_.write(b, 4);
        put_be(b, h.max_hash, 8); out_.write(b, 8);
        memset(b, 0, 52); out_.write(b, 52);
    }

    void write_code(uint64_t code) { write_code_with_taxid(code, 0); }

    void write_code_with_taxid(uint64_t code, uint32_t taxid) {
        write_header();
        const bool tx = h.is_include_taxid();
        if (!h.is_sorted()) {
            uint8_t b[12];
            const int n = h.is_compact() ? (h.k + 3) / 4 : 8;
            put_be(b, code, n);
            int m = n;
            if (tx) { put_be(b + n, taxid, h.taxid_bytes); m += h.taxid_bytes; }
            push(b, m);
            return;
        }
        if (!have_first_) {
            first_ = code;
            first_taxid_ = taxid;
            have_first_ = true;
            return;
        }
        if (first_ < prev_ || code < first_) throw Error("codes written to a sorted .unik must be ascending");
        uint8_t b[32];
        const uint64_t d0 = first_ - prev_, d1 = code - first_;
        const int l0 = byte_len(d0), l1 = byte_len(d1);
        b[0] = (uint8_t)(((l0 - 1) << 3) | (l1 - 1));
        put_be(b + 1, d0, l0);
        put_be(b + 1 + l0, d1, l1);
        int m = 1 + l0 + l1;
        if (tx) {
            put_be(b + m, first_taxid_, h.taxid_bytes); m += h.taxid_bytes;
            put_be(b + m, taxid, h.taxid_bytes); m += h.taxid_bytes;
        }
        push(b, m);
        prev_ = code;
        have_first_ = false;
    }

    // bulk: the header, then an encoded body (what ukm_unik_encode gives) as it is.  Not to be mixed with write_code().
    void write_body(const uint8_t *body, size_t n) {
        write_header();
        out_.write(body, n);
    }

    // the same for a stream in device-gzip mode: the body arrives deflated (OutStream::write_deflated)
    bool device_gzip() const { return out_.device_gzip(); }
    void write_body_deflated(const uint8_t *fragment, size_t n, uint32_t crc_of_body, uint64_t body_len) {
        write_header();
        out_.write_deflated(fragment, n, crc_of_body, body_len);
    }

    void flush() {
        write_header();
        if (h.is_sorted() && have_first_) {
            uint8_t b[16];
            b[0] = 128;
            put_be(b + 1, first_, 8);
            int m = 9;
            if (h.is_include_taxid()) { put_be(b + m, first_taxid_, h.taxid_bytes); m += h.taxid_bytes; }
            push(b, m);
            have_first_ = false;
        }
        if (!buf_.empty()) { out_.write(buf_.data(), buf_.size()); buf_.clear(); }
    }

  private:
    void push(const uint8_t *b, int n) {
        buf_.insert(buf_.end(), b, b + n);
        if (buf_.size() >= (1u << 20)) { out_.write(buf_.data(), buf_.size()); buf_.clear(); }
    }
    OutStream &out_;
    std::vector<uint8_t> buf_;
    bool wrote_header_ = false, have_first_ = false;
    uint64_t prev_ = 0, first_ = 0;
    uint32_t first_taxid_ = 0;
};

}  // namespace unik
