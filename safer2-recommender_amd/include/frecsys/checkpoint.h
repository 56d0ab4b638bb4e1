// checkpoint.h -- model checkpoints: the file format (version 1), its writer,
// reader and validation, and the capture / restore of a model's state.
//
// Two parts.  The HOST PART (everything up to FRECSYS_CHECKPOINT_HOST_ONLY's
// #ifndef) knows the layout and nothing else: no HIP, no frecsys_hip.h, plain
// g++.  The MODEL PART moves the state of a detail::DeviceModel between the
// device and a file through the host part.  tools/model_capi.cc and
// tools/run_model.cc go through this header; neither knows the layout.
//
// ---------------------------------------------------------------------------
// The file, version 1.  Little-endian; every offset and length is a u64.
//
//   offset  type      content
//        0  char[8]   magic "FRECSYS1"
//        8  u32       version = 1
//       12  u32       n_sections
//       16  u64       total file bytes (= end of the last section)
//       24  u64       flags (bit 0: the file holds the training tuples)
//       32  u64       checksum of the directory bytes
//       40  u8[24]    zero
//       64  directory n_sections x 32 B: char[8] tag (zero padded),
//                     u64 offset, u64 bytes, u64 checksum of the section
//
// The sections follow the directory.  Each starts at a multiple of 64, none
// overlap, every byte between them is zero, the file ends with the last one.
//
// Checksum of a byte range: zero-pad it to a multiple of 8, read it as u64
// words w_0 .. w_{m-1}; the checksum is
//     sum_i mix(w_i + (i + 1) * 0x9E3779B97F4A7C15)   mod 2^64
// with mix the splitmix64 finaliser
//     z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
//     z *= 0x94D049BB133111EB; z ^= z >> 31.
// A sum: any split over threads gives the same value.  An empty range is 0.
//
// Sections (tags are upper case, at most 8 bytes):
//   CONFIG  UTF-8 `name=value` lines ('\n' ends each): the fields of
//           frecsys_model_config except device / world / rank / comm_id, in
//           its order (dim, l2_reg, l2_reg_exp, uobs_weight, stdev, alpha,
//           bandwidth, stepsize, sampling_ratio, block_size, xi_iterations,
//           pd_iterations, use_epanechnikov, use_snr, print_train_stats,
//           print_residual_stats, print_var_stats, seed, parity_quirks,
//           use_cg, cg_error_tolerance, cg_max_iterations), floats as %.9g,
//           then model_name, n_users, n_items, n_tuples, epochs_trained and
//           tuples_checksum (decimal u64: the checksum of the USERS bytes
//           followed by the ITEMS bytes as ONE range; present also when the
//           tuples are left out).  Unknown names are ignored by a reader.
//   USERS, ITEMS  int32[n_tuples] each, the training tuples in file order;
//           present exactly when flag bit 0 is set.
//   U, V    float32 [n_users x dim] / [n_items x dim], row-major, no padding.
//   LOSS    float32 [n_users]: the user losses (every model has the vector).
//   OMEGA   float32 [n_users], ITEMREG float32 [n_items]: the dual weights
//           and the item regulariser of safer2, safer2pp, erm_mf, cvar_mf
//           (both required there, both absent for ials / ialspp).
//   STATE   `name=value` lines, the rest of the state that lives across
//           Train() calls; a name a model does not use is absent:
//             xi_bits       the float xi (prev_xi_) as its u32 bit pattern,
//                           decimal (safer2, safer2pp, cvar_mf)
//             weight_epoch  u64, the tag of the last weighted Gramian
//                           (safer2, safer2pp, erm_mf, cvar_mf)
//             snr_rng       the std::mt19937 of the SNR subsampling as
//                           operator<< writes it: 624 words and the position,
//                           blank separated (safer2, safer2pp)
//             snr_pending   blank separated indices already drawn from
//                           snr_rng for the next ComputeXi and not consumed
//                           yet (absent when none are pending: between two
//                           Train() calls none are)
// Required: CONFIG, U, V, LOSS, STATE.  No other tag is valid in version 1.
//
// Not stored, because they are functions of the tables and the tuples and the
// existing set / Gramian / load paths rebuild them with the same bits:
// Gramians, snapshots, the history-space basis, the LPT queue, the pre-split
// wide table, both CSR orientations, |H_u|, and the iALS++ / SAFER2++
// prediction vector (every Train() starts with PredictDataset).
// ---------------------------------------------------------------------------
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "frecsys/parallel.h"

namespace frecsys {
namespace checkpoint {

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__,
              "the checkpoint format is little-endian and is read and written in place");

// FRECSYS_OK / FRECSYS_ERR_INVALID / FRECSYS_ERR_IO (frecsys_hip.h)
enum Status { kOk = 0, kInvalid = 1, kIo = 8 };

constexpr uint32_t kVersion = 1;
constexpr uint64_t kFlagTuples = 1;
constexpr uint64_t kHeaderBytes = 64, kEntryBytes = 32, kAlign = 64;
constexpr uint32_t kMaxSections = 64;
constexpr uint64_t kMaxTextBytes = 1 << 20;  // CONFIG / STATE
constexpr int32_t kMaxDim = 1024;            // the widest kernel built

inline uint64_t mix64(uint64_t z) {
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// The checksum of a byte range given in pieces.
class Checksum {
 public:
  void Update(const void* data, uint64_t bytes) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    while (npend_ && bytes) {  // complete the word a previous piece left open
      pend_[npend_++] = *p++;
      --bytes;
      if (npend_ == 8) Flush();
    }
    const uint64_t words = bytes / 8, first = words_;
    if (words) {
      std::atomic<uint64_t> total{0};
      ThreadPool::Get().ParallelFor((int64_t)words, 1 << 16, [&](int64_t lo, int64_t hi) {
        uint64_t s = 0;
        for (int64_t i = lo; i < hi; ++i) {
          uint64_t w;
          std::memcpy(&w, p + 8 * (uint64_t)i, 8);
          s += mix64(w + (first + (uint64_t)i + 1) * 0x9E3779B97F4A7C15ull);
        }
        total.fetch_add(s, std::memory_order_relaxed);
      });
      sum_ += total.load();
      words_ += words;
    }
    for (uint64_t i = words * 8; i < bytes; ++i) pend_[npend_++] = p[i];
  }
  uint64_t Finish() {
    if (npend_) {
      while (npend_ < 8) pend_[npend_++] = 0;
      Flush();
    }
    return sum_;
  }
  static uint64_t Of(const void* data, uint64_t bytes) {
    Checksum c;
    c.Update(data, bytes);
    return c.Finish();
  }

 private:
  void Flush() {
    uint64_t w;
    std::memcpy(&w, pend_, 8);
    sum_ += mix64(w + (++words_) * 0x9E3779B97F4A7C15ull);
    npend_ = 0;
  }
  uint64_t sum_ = 0, words_ = 0;
  unsigned char pend_[8] = {0};
  int npend_ = 0;
};

// CONFIG's tuples_checksum: USERS bytes followed by ITEMS bytes, one range.
inline uint64_t TuplesChecksum(const int32_t* users, const int32_t* items, int64_t n) {
  Checksum c;
  c.Update(users, (uint64_t)n * 4);
  c.Update(items, (uint64_t)n * 4);
  return c.Finish();
}

// The stored fields of frecsys_model_config (run_model's defaults).
struct Config {
  std::string model_name;
  int32_t dim = 8;
  float l2_reg = 0.002f, l2_reg_exp = 1.0f, uobs_weight = 0.1f, stdev = 0.1f, alpha = 0.3f,
        bandwidth = 1.0f, stepsize = 0.1f, sampling_ratio = 0.1f;
  int32_t block_size = 64, xi_iterations = 5, pd_iterations = 1, use_epanechnikov = 0,
          use_snr = 0, print_train_stats = 1, print_residual_stats = 0, print_var_stats = 0;
  int64_t seed = -1;
  int32_t parity_quirks = 1, use_cg = 0;
  float cg_error_tolerance = 1e-10f;
  int32_t cg_max_iterations = 100;
};

struct Info {
  Config config;
  int64_t n_users = 0, n_items = 0, n_tuples = 0, epochs_trained = 0;
  uint64_t flags = 0, tuples_checksum = 0;
  uint32_t version = 0;
};

inline bool IsModelName(const std::string& s) {
  for (const char* m : {"ials", "ialspp", "safer2", "safer2pp", "cvar_mf", "erm_mf"})
    if (s == m) return true;
  return false;
}
inline bool HasDualState(const std::string& model) { return model != "ials" && model != "ialspp"; }

using KeyValues = std::map<std::string, std::string>;

namespace detail {

// The one list of the stored numeric fields, in file order.  Config,
// frecsys_model_config and ModelParams name them alike, so the list walks two
// objects at once: f(name, a.field, b.field).  seed and parity_quirks are
// options of the device context and not in ModelParams: they are visited when
// both objects have them.
template <class T, class = void>
struct HasSeed : std::false_type {};
template <class T>
struct HasSeed<T, std::void_t<decltype(std::declval<T&>().seed)>> : std::true_type {};

template <class A, class B, class F>
void ForEachConfigField(A& a, B& b, F&& f) {
  f("dim", a.dim, b.dim);
  f("l2_reg", a.l2_reg, b.l2_reg);
  f("l2_reg_exp", a.l2_reg_exp, b.l2_reg_exp);
  f("uobs_weight", a.uobs_weight, b.uobs_weight);
  f("stdev", a.stdev, b.stdev);
  f("alpha", a.alpha, b.alpha);
  f("bandwidth", a.bandwidth, b.bandwidth);
  f("stepsize", a.stepsize, b.stepsize);
  f("sampling_ratio", a.sampling_ratio, b.sampling_ratio);
  f("block_size", a.block_size, b.block_size);
  f("xi_iterations", a.xi_iterations, b.xi_iterations);
  f("pd_iterations", a.pd_iterations, b.pd_iterations);
  f("use_epanechnikov", a.use_epanechnikov, b.use_epanechnikov);
  f("use_snr", a.use_snr, b.use_snr);
  f("print_train_stats", a.print_train_stats, b.print_train_stats);
  f("print_residual_stats", a.print_residual_stats, b.print_residual_stats);
  f("print_var_stats", a.print_var_stats, b.print_var_stats);
  if constexpr (HasSeed<A>::value && HasSeed<B>::value) {
    f("seed", a.seed, b.seed);
    f("parity_quirks", a.parity_quirks, b.parity_quirks);
  }
  f("use_cg", a.use_cg, b.use_cg);
  f("cg_error_tolerance", a.cg_error_tolerance, b.cg_error_tolerance);
  f("cg_max_iterations", a.cg_max_iterations, b.cg_max_iterations);
}
// f(name, field) for every numeric CONFIG field, in file order.
template <class C, class F>
void ForEachConfigField(C& c, F&& f) {
  ForEachConfigField(c, c, [&f](const char* n, auto& x, auto&) { f(n, x); });
}

struct FieldWriter {
  std::string* out;
  void operator()(const char* n, const int32_t& v) const { *out += std::string(n) + "=" + std::to_string(v) + "\n"; }
  void operator()(const char* n, const int64_t& v) const { *out += std::string(n) + "=" + std::to_string(v) + "\n"; }
  void operator()(const char* n, const float& v) const {
    char b[48];
    snprintf(b, sizeof(b), "%.9g", (double)v);
    *out += std::string(n) + "=" + b + "\n";
  }
};

inline bool parse_i64(const std::string& s, int64_t* v) {
  if (s.empty()) return false;
  errno = 0;
  char* e = nullptr;
  const long long x = strtoll(s.c_str(), &e, 10);
  if (errno || *e) return false;
  *v = x;
  return true;
}
inline bool parse_u64(const std::string& s, uint64_t* v) {
  if (s.empty() || s[0] == '-' || s[0] == '+') return false;
  errno = 0;
  char* e = nullptr;
  const unsigned long long x = strtoull(s.c_str(), &e, 10);
  if (errno || *e) return false;
  *v = x;
  return true;
}

struct FieldReader {
  const KeyValues* kv;
  std::string* err;
  const std::string* find(const char* n) const {
    auto it = kv->find(n);
    if (it == kv->end()) {
      if (err->empty()) *err = std::string("CONFIG lacks ") + n;
      return nullptr;
    }
    return &it->second;
  }
  void bad(const char* n, const std::string& s) const {
    if (err->empty()) *err = std::string("CONFIG: bad value of ") + n + ": '" + s + "'";
  }
  void operator()(const char* n, int32_t& v) const {
    int64_t x;
    if (const std::string* s = find(n)) {
      if (!parse_i64(*s, &x) || x < INT32_MIN || x > INT32_MAX) return bad(n, *s);
      v = (int32_t)x;
    }
  }
  void operator()(const char* n, int64_t& v) const {
    if (const std::string* s = find(n))
      if (!parse_i64(*s, &v)) bad(n, *s);
  }
  void operator()(const char* n, float& v) const {
    if (const std::string* s = find(n)) {
      char* e = nullptr;
      const float x = s->empty() ? 0.0f : strtof(s->c_str(), &e);
      if (s->empty() || *e) return bad(n, *s);
      v = x;
    }
  }
};

inline std::string tag_string(const char* tag8) {
  size_t n = 0;
  while (n < 8 && tag8[n]) ++n;
  return std::string(tag8, n);
}

}  // namespace detail

// to->field = from.field for every field of the list that both have, converted
// to the field's type: a flag kept as an int becomes a bool by != 0, a bool 0 / 1.
template <class From, class To>
void CopyConfigFields(const From& from, To* to) {
  detail::ForEachConfigField(from, *to, [](const char*, const auto& s, auto& d) {
    d = static_cast<std::decay_t<decltype(d)>>(s);
  });
}

// `name=value` lines <-> a map.  A line without '=' or an empty name is an
// error; a repeated name keeps its last value.
inline bool ParseKeyValues(const std::string& text, KeyValues* kv, std::string* err) {
  size_t pos = 0;
  while (pos < text.size()) {
    size_t nl = text.find('\n', pos);
    if (nl == std::string::npos) nl = text.size();
    const std::string line = text.substr(pos, nl - pos);
    pos = nl + 1;
    if (line.empty()) continue;
    const size_t eq = line.find('=');
    if (eq == std::string::npos || eq == 0) {
      *err = "line without name=value: '" + line.substr(0, 40) + "'";
      return false;
    }
    (*kv)[line.substr(0, eq)] = line.substr(eq + 1);
  }
  return true;
}
inline std::string FormatKeyValues(const KeyValues& kv) {
  std::string s;
  for (const auto& e : kv) s += e.first + "=" + e.second + "\n";
  return s;
}

inline std::string FormatConfig(const Info& in) {
  std::string s;
  detail::ForEachConfigField(in.config, detail::FieldWriter{&s});
  s += "model_name=" + in.config.model_name + "\n";
  s += "n_users=" + std::to_string(in.n_users) + "\n";
  s += "n_items=" + std::to_string(in.n_items) + "\n";
  s += "n_tuples=" + std::to_string(in.n_tuples) + "\n";
  s += "epochs_trained=" + std::to_string(in.epochs_trained) + "\n";
  s += "tuples_checksum=" + std::to_string(in.tuples_checksum) + "\n";
  return s;
}

// CONFIG's text into `in` (config and the counts), with the range checks that
// need no other section.  false + *err on a problem.
inline bool ParseConfig(const std::string& text, Info* in, std::string* err) {
  KeyValues kv;
  std::string e;
  if (!ParseKeyValues(text, &kv, &e)) {
    *err = "CONFIG: " + e;
    return false;
  }
  const detail::FieldReader rd{&kv, &e};
  detail::ForEachConfigField(in->config, rd);
  if (const std::string* s = rd.find("model_name")) in->config.model_name = *s;
  rd("n_users", in->n_users);
  rd("n_items", in->n_items);
  rd("n_tuples", in->n_tuples);
  rd("epochs_trained", in->epochs_trained);
  if (const std::string* s = rd.find("tuples_checksum"))
    if (!detail::parse_u64(*s, &in->tuples_checksum)) rd.bad("tuples_checksum", *s);
  if (!e.empty()) {
    *err = e;
    return false;
  }
  if (!IsModelName(in->config.model_name)) {
    *err = "CONFIG: unknown model_name '" + in->config.model_name.substr(0, 32) + "'";
    return false;
  }
  if (in->config.dim < 1 || in->config.dim > kMaxDim) {
    *err = "CONFIG: dim=" + std::to_string(in->config.dim) + " is outside [1, " +
           std::to_string(kMaxDim) + "]";
    return false;
  }
  if (in->n_users < 1 || in->n_users > INT32_MAX || in->n_items < 1 || in->n_items > INT32_MAX) {
    *err = "CONFIG: n_users / n_items outside [1, 2^31)";
    return false;
  }
  if (in->n_tuples < 1 || in->n_tuples > INT32_MAX || in->epochs_trained < 0) {
    *err = "CONFIG: n_tuples outside [1, 2^31) or negative epochs_trained";
    return false;
  }
  return true;
}

struct Section {
  std::string tag;
  uint64_t offset = 0, bytes = 0, checksum = 0;
};

// Reads and validates one file.  Nothing is allocated or read before its
// length and offset were checked against the file size, and no allocation
// grows with a number the file states except the two text sections (capped
// at kMaxTextBytes); payloads are read in fixed chunks or into the caller's
// buffer.
class Reader {
 public:
  Reader() = default;
  ~Reader() { Close(); }
  Reader(const Reader&) = delete;
  Reader& operator=(const Reader&) = delete;

  // verify = false: header, directory (bounds, alignment, overlap, tags,
  // sizes against CONFIG) and CONFIG; verify = true: also every section's
  // checksum, the zero gaps, the tuple ids and tuples_checksum, and STATE's
  // syntax.
  Status Open(const std::string& path, bool verify, std::string* err) {
    Close();
    std::string unused;
    if (!err) err = &unused;
    path_ = path;
    fd_ = open(path.c_str(), O_RDONLY | O_CLOEXEC);
    if (fd_ < 0) return Fail(kIo, "cannot open " + path + ": " + strerror(errno), err);
    struct stat st;
    if (fstat(fd_, &st) != 0) return Fail(kIo, "cannot stat " + path + ": " + strerror(errno), err);
    if (!S_ISREG(st.st_mode)) return Fail(kInvalid, path + " is not a regular file", err);
    size_ = (uint64_t)st.st_size;
    const Status s = Validate(verify, err);
    if (s != kOk) Close();
    return s;
  }
  void Close() {
    if (fd_ >= 0) close(fd_);
    fd_ = -1;
    sections_.clear();
  }

  const Info& info() const { return info_; }
  const std::vector<Section>& sections() const { return sections_; }
  const Section* Find(const std::string& tag) const {
    for (const Section& s : sections_)
      if (s.tag == tag) return &s;
    return nullptr;
  }
  bool has_tuples() const { return (info_.flags & kFlagTuples) != 0; }

  // The first `bytes` bytes of a section into dst (bytes <= its size).
  Status Read(const std::string& tag, void* dst, uint64_t bytes, std::string* err) const {
    const Section* s = Find(tag);
    if (!s) return Fail(kInvalid, "section " + tag + " is missing", err);
    if (bytes > s->bytes) return Fail(kInvalid, "section " + tag + " is shorter than asked", err);
    return ReadAt(s->offset, dst, bytes, err);
  }
  Status ReadText(const std::string& tag, std::string* out, std::string* err) const {
    const Section* s = Find(tag);
    if (!s) return Fail(kInvalid, "section " + tag + " is missing", err);
    if (s->bytes > kMaxTextBytes) return Fail(kInvalid, "section " + tag + " is too large", err);
    out->resize((size_t)s->bytes);
    return ReadAt(s->offset, out->empty() ? nullptr : &(*out)[0], s->bytes, err);
  }

 private:
  static Status Fail(Status s, const std::string& msg, std::string* err) {
    if (err) *err = msg;
    return s;
  }
  Status ReadAt(uint64_t off, void* dst, uint64_t bytes, std::string* err) const {
    if (off > size_ || bytes > size_ - off)
      return Fail(kInvalid, "read past the end of " + path_, err);
    unsigned char* p = static_cast<unsigned char*>(dst);
    while (bytes) {
      const ssize_t r = pread(fd_, p, (size_t)std::min<uint64_t>(bytes, 1u << 30), (off_t)off);
      if (r < 0 && errno == EINTR) continue;
      if (r < 0) return Fail(kIo, "read of " + path_ + " failed: " + strerror(errno), err);
      if (r == 0) return Fail(kInvalid, path_ + " shrank while it was read", err);
      p += r;
      off += (uint64_t)r;
      bytes -= (uint64_t)r;
    }
    return kOk;
  }
  static uint64_t U64(const unsigned char* p) {
    uint64_t v;
    std::memcpy(&v, p, 8);
    return v;
  }
  static uint32_t U32(const unsigned char* p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
  }

  Status Validate(bool verify, std::string* err) {
    const std::string w = path_ + ": ";
    if (size_ < kHeaderBytes)
      return Fail(kInvalid, w + "truncated: " + std::to_string(size_) + " bytes, the header has 64", err);
    unsigned char h[kHeaderBytes];
    Status s = ReadAt(0, h, kHeaderBytes, err);
    if (s != kOk) return s;
    if (std::memcmp(h, "FRECSYS1", 8) != 0) return Fail(kInvalid, w + "bad magic (not a checkpoint)", err);
    info_ = Info();
    info_.version = U32(h + 8);
    if (info_.version != kVersion)
      return Fail(kInvalid, w + "version " + std::to_string(info_.version) + " is not supported (1 is)", err);
    const uint32_t n = U32(h + 12);
    if (n < 1 || n > kMaxSections)
      return Fail(kInvalid, w + "n_sections " + std::to_string(n) + " is outside [1, 64]", err);
    const uint64_t total = U64(h + 16);
    if (total != size_)
      return Fail(kInvalid, w + "the header states " + std::to_string(total) + " bytes, the file has " +
                                std::to_string(size_) + " (truncated or extended)", err);
    info_.flags = U64(h + 24);
    if (info_.flags & ~kFlagTuples) return Fail(kInvalid, w + "unknown flag bits", err);
    for (int i = 40; i < 64; ++i)
      if (h[i]) return Fail(kInvalid, w + "reserved header bytes are not zero", err);
    const uint64_t dir_end = kHeaderBytes + kEntryBytes * n;
    if (dir_end > size_) return Fail(kInvalid, w + "truncated inside the directory", err);
    std::vector<unsigned char> dir((size_t)(kEntryBytes * n));
    if ((s = ReadAt(kHeaderBytes, dir.data(), dir.size(), err)) != kOk) return s;
    if (Checksum::Of(dir.data(), dir.size()) != U64(h + 32))
      return Fail(kInvalid, w + "directory checksum mismatch", err);
    sections_.clear();
    for (uint32_t i = 0; i < n; ++i) {
      const unsigned char* e = dir.data() + kEntryBytes * i;
      Section sec;
      sec.tag = detail::tag_string(reinterpret_cast<const char*>(e));
      for (size_t k = sec.tag.size(); k < 8; ++k)
        if (e[k]) return Fail(kInvalid, w + "section tag " + std::to_string(i) + " is not zero padded", err);
      sec.offset = U64(e + 8);
      sec.bytes = U64(e + 16);
      sec.checksum = U64(e + 24);
      const std::string t = "section " + sec.tag + ": ";
      if (!KnownTag(sec.tag)) return Fail(kInvalid, w + "unknown section tag '" + sec.tag + "'", err);
      if (Find(sec.tag)) return Fail(kInvalid, w + t + "listed twice", err);
      if (sec.offset % kAlign) return Fail(kInvalid, w + t + "offset is not a multiple of 64", err);
      if (sec.offset < dir_end) return Fail(kInvalid, w + t + "offset lies inside the directory", err);
      if (sec.offset > size_) return Fail(kInvalid, w + t + "offset is past the end of the file", err);
      if (sec.bytes > size_ - sec.offset)  // no offset + bytes: it may wrap
        return Fail(kInvalid, w + t + "offset + bytes is past the end of the file", err);
      sections_.push_back(sec);
    }
    std::vector<const Section*> by_off;
    // an empty section (iALS's STATE) holds no byte and overlaps nothing
    for (const Section& x : sections_) by_off.push_back(&x);
    std::sort(by_off.begin(), by_off.end(), [](const Section* a, const Section* b) {
      return a->offset != b->offset ? a->offset < b->offset : a->bytes < b->bytes;
    });
    uint64_t end = dir_end;
    const Section* prev = nullptr;
    for (const Section* x : by_off) {
      if (!x->bytes) continue;
      if (prev && x->offset < end)
        return Fail(kInvalid, w + "sections " + prev->tag + " and " + x->tag + " overlap", err);
      prev = x;
      end = x->offset + x->bytes;
    }
    for (const Section* x : by_off) end = std::max(end, x->offset);
    if (end != size_) return Fail(kInvalid, w + "bytes after the last section", err);

    // CONFIG (its checksum always: it is read anyway)
    std::string text;
    if (!Find("CONFIG")) return Fail(kInvalid, w + "section CONFIG is missing", err);
    if ((s = ReadText("CONFIG", &text, err)) != kOk) return s == kInvalid ? Fail(s, w + *err, err) : s;
    if (Checksum::Of(text.data(), text.size()) != Find("CONFIG")->checksum)
      return Fail(kInvalid, w + "section CONFIG: checksum mismatch", err);
    std::string e;
    if (!ParseConfig(text, &info_, &e)) return Fail(kInvalid, w + e, err);

    // the sections a model of this CONFIG has, and their sizes
    const Config& c = info_.config;
    const uint64_t nu = (uint64_t)info_.n_users, ni = (uint64_t)info_.n_items,
                   nt = (uint64_t)info_.n_tuples, d = (uint64_t)c.dim;
    const bool dual = HasDualState(c.model_name);
    struct Want {
      const char* tag;
      bool present;
      uint64_t bytes;
      const char* shape;
    };
    const Want want[] = {{"U", true, nu * d * 4, "n_users * dim * 4"},
                         {"V", true, ni * d * 4, "n_items * dim * 4"},
                         {"LOSS", true, nu * 4, "n_users * 4"},
                         {"OMEGA", dual, nu * 4, "n_users * 4"},
                         {"ITEMREG", dual, ni * 4, "n_items * 4"},
                         {"USERS", has_tuples(), nt * 4, "n_tuples * 4"},
                         {"ITEMS", has_tuples(), nt * 4, "n_tuples * 4"}};
    for (const Want& x : want) {
      const Section* sec = Find(x.tag);
      if (x.present && !sec) return Fail(kInvalid, w + "section " + x.tag + " is missing", err);
      if (!x.present && sec)
        return Fail(kInvalid, w + "section " + x.tag + " does not belong in this file (model " +
                                  c.model_name + ", flags " + std::to_string(info_.flags) + ")", err);
      if (sec && sec->bytes != x.bytes)
        return Fail(kInvalid, w + "section " + x.tag + " has " + std::to_string(sec->bytes) +
                                  " bytes, " + x.shape + " = " + std::to_string(x.bytes), err);
    }
    if (!Find("STATE")) return Fail(kInvalid, w + "section STATE is missing", err);
    if (Find("STATE")->bytes > kMaxTextBytes) return Fail(kInvalid, w + "section STATE is too large", err);
    if (!verify) return kOk;

    // checksums, gaps, tuple ids
    uint64_t pos = dir_end;
    for (const Section* sec : by_off) {
      if ((s = CheckGap(pos, sec->offset, err)) != kOk) return s;
      pos = std::max(pos, sec->offset + sec->bytes);
    }
    Checksum tuples;
    for (const char* tag : {"CONFIG", "STATE", "U", "V", "LOSS", "OMEGA", "ITEMREG", "USERS", "ITEMS"}) {
      const Section* sec = Find(tag);
      if (!sec) continue;
      const std::string t(tag);
      const int64_t id_limit = t == "USERS" ? info_.n_users : t == "ITEMS" ? info_.n_items : 0;
      if ((s = CheckSection(*sec, id_limit, id_limit ? &tuples : nullptr, err)) != kOk) return s;
    }
    if (has_tuples() && tuples.Finish() != info_.tuples_checksum)
      return Fail(kInvalid, w + "tuples_checksum of CONFIG does not match USERS + ITEMS", err);
    if ((s = ReadText("STATE", &text, err)) != kOk) return s;
    KeyValues kv;
    if (!ParseKeyValues(text, &kv, &e)) return Fail(kInvalid, w + "STATE: " + e, err);
    return kOk;
  }

  static bool KnownTag(const std::string& t) {
    for (const char* k : {"CONFIG", "STATE", "U", "V", "LOSS", "OMEGA", "ITEMREG", "USERS", "ITEMS"})
      if (t == k) return true;
    return false;
  }

  static constexpr size_t kChunk = 4u << 20;  // a multiple of 8

  Status CheckGap(uint64_t from, uint64_t to, std::string* err) {
    std::vector<unsigned char> buf;
    while (from < to) {
      const uint64_t n = std::min<uint64_t>(to - from, kChunk);
      buf.resize((size_t)n);
      const Status s = ReadAt(from, buf.data(), n, err);
      if (s != kOk) return s;
      for (unsigned char b : buf)
        if (b) return Fail(kInvalid, path_ + ": a byte between two sections is not zero", err);
      from += n;
    }
    return kOk;
  }

  // One pass over a section: its checksum and, for USERS / ITEMS, the ids.
  Status CheckSection(const Section& sec, int64_t id_limit, Checksum* tuples, std::string* err) {
    std::vector<unsigned char> buf((size_t)std::min<uint64_t>(sec.bytes, kChunk));
    Checksum c;
    for (uint64_t done = 0; done < sec.bytes;) {
      const uint64_t n = std::min<uint64_t>(sec.bytes - done, kChunk);
      const Status s = ReadAt(sec.offset + done, buf.data(), n, err);
      if (s != kOk) return s;
      c.Update(buf.data(), n);
      if (tuples) tuples->Update(buf.data(), n);
      if (id_limit)
        for (uint64_t k = 0; k + 4 <= n; k += 4) {
          int32_t id;
          std::memcpy(&id, buf.data() + k, 4);
          if (id < 0 || id >= id_limit)
            return Fail(kInvalid, path_ + ": section " + sec.tag + ": id " + std::to_string(id) +
                                      " of tuple " + std::to_string((done + k) / 4) + " is outside [0, " +
                                      std::to_string(id_limit) + ")", err);
        }
      done += n;
    }
    if (c.Finish() != sec.checksum)
      return Fail(kInvalid, path_ + ": section " + sec.tag + ": checksum mismatch", err);
    return kOk;
  }

  std::string path_;
  int fd_ = -1;
  uint64_t size_ = 0;
  Info info_;
  std::vector<Section> sections_;
};

// Writes one file: Begin() with every section's tag and size, Write() each
// section once (any order), Commit().  The bytes go to `path` + a temporary
// suffix; Commit() flushes, fsyncs, renames over `path` and fsyncs the
// directory.  Anything short of a finished Commit() removes the temporary
// file and leaves an existing `path` as it was.
class Writer {
 public:
  Writer() = default;
  ~Writer() { Abort(); }
  Writer(const Writer&) = delete;
  Writer& operator=(const Writer&) = delete;

  Status Begin(const std::string& path, uint64_t flags,
               const std::vector<std::pair<std::string, uint64_t>>& sections, std::string* err) {
    Abort();
    path_ = path;
    flags_ = flags;
    sections_.clear();
    written_.assign(sections.size(), false);
    if (sections.empty() || sections.size() > kMaxSections) return Fail(kInvalid, "bad section count", err);
    uint64_t pos = kHeaderBytes + kEntryBytes * sections.size();
    for (const auto& s : sections) {
      if (s.first.empty() || s.first.size() > 8) return Fail(kInvalid, "bad section tag", err);
      Section sec;
      sec.tag = s.first;
      sec.offset = (pos + kAlign - 1) / kAlign * kAlign;
      sec.bytes = s.second;
      pos = sec.offset + sec.bytes;
      sections_.push_back(sec);
    }
    total_ = pos;
    tmp_ = path + ".tmp." + std::to_string((long long)getpid());
    fd_ = open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd_ < 0) {
      const std::string e = strerror(errno);
      tmp_.clear();
      return Fail(kIo, "cannot create " + path + ".tmp.*: " + e, err);
    }
    return kOk;
  }

  Status Write(const std::string& tag, const void* data, uint64_t bytes, std::string* err) {
    for (size_t i = 0; i < sections_.size(); ++i) {
      if (sections_[i].tag != tag) continue;
      if (written_[i] || bytes != sections_[i].bytes)
        return Fail(kInvalid, "section " + tag + " written twice or with another size", err);
      sections_[i].checksum = Checksum::Of(data, bytes);
      written_[i] = true;
      return WriteAt(sections_[i].offset, data, bytes, err);
    }
    return Fail(kInvalid, "section " + tag + " was not announced", err);
  }

  Status Commit(std::string* err) {
    if (fd_ < 0) return Fail(kInvalid, "no open checkpoint", err);
    for (size_t i = 0; i < sections_.size(); ++i)
      if (!written_[i]) return Fail(kInvalid, "section " + sections_[i].tag + " was not written", err);
    std::vector<unsigned char> head((size_t)(kHeaderBytes + kEntryBytes * sections_.size()), 0);
    for (size_t i = 0; i < sections_.size(); ++i) {
      unsigned char* e = head.data() + kHeaderBytes + kEntryBytes * i;
      std::memcpy(e, sections_[i].tag.data(), sections_[i].tag.size());
      std::memcpy(e + 8, &sections_[i].offset, 8);
      std::memcpy(e + 16, &sections_[i].bytes, 8);
      std::memcpy(e + 24, &sections_[i].checksum, 8);
    }
    const uint32_t version = kVersion, n = (uint32_t)sections_.size();
    const uint64_t dsum = Checksum::Of(head.data() + kHeaderBytes, head.size() - kHeaderBytes);
    std::memcpy(head.data(), "FRECSYS1", 8);
    std::memcpy(head.data() + 8, &version, 4);
    std::memcpy(head.data() + 12, &n, 4);
    std::memcpy(head.data() + 16, &total_, 8);
    std::memcpy(head.data() + 24, &flags_, 8);
    std::memcpy(head.data() + 32, &dsum, 8);
    Status s = WriteAt(0, head.data(), head.size(), err);
    if (s != kOk) return s;
    // a last section of 0 bytes, or holes: the file has its stated length
    if (ftruncate(fd_, (off_t)total_) != 0 || fsync(fd_) != 0) {
      const std::string e = strerror(errno);
      Abort();
      return Fail(kIo, "cannot flush " + tmp_ + ": " + e, err);
    }
    if (close(fd_) != 0) {
      const std::string e = strerror(errno);
      fd_ = -1;
      Abort();
      return Fail(kIo, "cannot close the temporary file: " + e, err);
    }
    fd_ = -1;
    if (rename(tmp_.c_str(), path_.c_str()) != 0) {
      const std::string e = strerror(errno);
      Abort();
      return Fail(kIo, "cannot rename onto " + path_ + ": " + e, err);
    }
    tmp_.clear();
    const size_t slash = path_.rfind('/');
    const std::string dir = slash == std::string::npos ? "." : slash == 0 ? "/" : path_.substr(0, slash);
    const int dfd = open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
    if (dfd >= 0) {
      fsync(dfd);
      close(dfd);
    }
    return kOk;
  }

  void Abort() {
    if (fd_ >= 0) close(fd_);
    fd_ = -1;
    if (!tmp_.empty()) unlink(tmp_.c_str());
    tmp_.clear();
  }

 private:
  static Status Fail(Status s, const std::string& msg, std::string* err) {
    if (err) *err = msg;
    return s;
  }
  Status WriteAt(uint64_t off, const void* data, uint64_t bytes, std::string* err) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    while (bytes) {
      const ssize_t r = pwrite(fd_, p, (size_t)std::min<uint64_t>(bytes, 1u << 30), (off_t)off);
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) {
        const std::string e = strerror(errno);
        Abort();
        return Fail(kIo, "write to " + path_ + ".tmp.* failed: " + e, err);
      }
      p += r;
      off += (uint64_t)r;
      bytes -= (uint64_t)r;
    }
    return kOk;
  }

  std::string path_, tmp_;
  int fd_ = -1;
  uint64_t flags_ = 0, total_ = 0;
  std::vector<Section> sections_;
  std::vector<bool> written_;
};

}  // namespace checkpoint
}  // namespace frecsys

// ===========================================================================
// MODEL PART: the state of a detail::DeviceModel <-> a file.
// ===========================================================================
#ifndef FRECSYS_CHECKPOINT_HOST_ONLY

#include "frecsys/factory.h"

namespace frecsys {
namespace checkpoint {

static_assert(kInvalid == FRECSYS_ERR_INVALID && kIo == FRECSYS_ERR_IO && kOk == FRECSYS_OK,
              "Status mirrors the C-ABI codes");

inline ModelParams ToParams(const Config& c) {
  ModelParams p;
  CopyConfigFields(c, &p);
  return p;
}
inline Config FromParams(const std::string& model_name, const ModelParams& p, int64_t seed,
                         bool parity_quirks) {
  Config c;
  c.model_name = model_name;
  CopyConfigFields(p, &c);
  c.seed = seed;
  c.parity_quirks = parity_quirks;
  return c;
}

// The tuples a file is written for: the arrays (nullptr: left out of the
// file) with their count and checksum (a model loaded without tuples passes
// the stored ones on).
struct Tuples {
  const int32_t* users = nullptr;
  const int32_t* items = nullptr;
  int64_t n = 0;
  uint64_t checksum = 0;
};

// Writes `dm` to `path`.  One table is on the host at a time.
inline Status SaveModel(const Config& config, frecsys::detail::DeviceModel* dm, const Tuples& t,
                        int64_t epochs_trained, const std::string& path, std::string* err) {
  Info in;
  in.config = config;
  in.n_users = dm->device().rows(DeviceContext::USER);
  in.n_items = dm->device().rows(DeviceContext::ITEM);
  in.n_tuples = t.n;
  in.epochs_trained = epochs_trained;
  in.tuples_checksum = t.checksum;
  const bool data = t.users && t.items;
  const bool dual = HasDualState(config.model_name);
  const std::string cfg_text = FormatConfig(in);
  KeyValues kv;
  dm->CaptureState(&kv);
  const std::string state_text = FormatKeyValues(kv);
  const uint64_t nu = (uint64_t)in.n_users, ni = (uint64_t)in.n_items, d = (uint64_t)config.dim;
  if ((uint64_t)dm->user_loss().size() != nu ||
      (dual && ((uint64_t)dm->dual_weights().size() != nu ||
                (uint64_t)dm->item_regularization().size() != ni))) {
    if (err) *err = "the model's host vectors do not have the table sizes";
    return kInvalid;
  }
  std::vector<std::pair<std::string, uint64_t>> lay = {{"CONFIG", cfg_text.size()},
                                                       {"STATE", state_text.size()}};
  if (data) {
    lay.push_back({"USERS", (uint64_t)t.n * 4});
    lay.push_back({"ITEMS", (uint64_t)t.n * 4});
  }
  lay.push_back({"LOSS", nu * 4});
  if (dual) {
    lay.push_back({"OMEGA", nu * 4});
    lay.push_back({"ITEMREG", ni * 4});
  }
  lay.push_back({"U", nu * d * 4});
  lay.push_back({"V", ni * d * 4});
  Writer w;
  Status s = w.Begin(path, data ? kFlagTuples : 0, lay, err);
  if (s == kOk) s = w.Write("CONFIG", cfg_text.data(), cfg_text.size(), err);
  if (s == kOk) s = w.Write("STATE", state_text.data(), state_text.size(), err);
  if (s == kOk && data) s = w.Write("USERS", t.users, (uint64_t)t.n * 4, err);
  if (s == kOk && data) s = w.Write("ITEMS", t.items, (uint64_t)t.n * 4, err);
  if (s == kOk) s = w.Write("LOSS", dm->user_loss().data(), nu * 4, err);
  if (s == kOk && dual) s = w.Write("OMEGA", dm->dual_weights().data(), nu * 4, err);
  if (s == kOk && dual) s = w.Write("ITEMREG", dm->item_regularization().data(), ni * 4, err);
  for (int side : {(int)DeviceContext::USER, (int)DeviceContext::ITEM}) {
    if (s != kOk) break;
    const MatrixXf m = dm->device().Get(side);
    s = w.Write(side == DeviceContext::USER ? "U" : "V", m.data(),
                (uint64_t)m.rows() * d * 4, err);
  }
  if (s == kOk) s = w.Commit(err);
  return s;
}

// Rows [0, stored n) of U and V from an open (verified) file into a model of
// at least the stored sizes and the file's dim; the other rows keep what
// they hold.  One table on the host at a time; the Gramians the model caches
// are rebuilt by its own set path.
inline Status RestoreTables(const Reader& r, frecsys::detail::DeviceModel* dm, std::string* err) {
  const Info& in = r.info();
  for (int side : {(int)DeviceContext::USER, (int)DeviceContext::ITEM}) {
    const int64_t stored = side == DeviceContext::USER ? in.n_users : in.n_items;
    const int64_t have = dm->device().rows(side);
    if (have < stored || dm->device().dim() != in.config.dim) {
      if (err) *err = "the model is smaller than the stored tables or has another dim";
      return kInvalid;
    }
    MatrixXf m = have == stored ? MatrixXf(have, in.config.dim) : dm->device().Get(side);
    const Status s = r.Read(side == DeviceContext::USER ? "U" : "V", m.data(),
                            (uint64_t)stored * (uint64_t)in.config.dim * 4, err);
    if (s != kOk) return s;
    dm->SetTable(side, m);
  }
  dm->TablesSet();
  return kOk;
}

// The whole saved state into a fresh model of the stored sizes: tables, the
// host vectors, STATE; with `train` (the saved run's tuples) also |H_u| and
// the training CSR on the device, so that the next Train() continues the run
// and exclude_seen works before it.
inline Status RestoreModel(const Reader& r, frecsys::detail::DeviceModel* dm, const Dataset* train,
                           std::string* err) {
  const Info& in = r.info();
  if (dm->device().rows(DeviceContext::USER) != in.n_users ||
      dm->device().rows(DeviceContext::ITEM) != in.n_items) {
    if (err) *err = "the model does not have the stored sizes";
    return kInvalid;
  }
  Status s = RestoreTables(r, dm, err);
  if (s != kOk) return s;
  const bool dual = HasDualState(in.config.model_name);
  std::vector<float> loss((size_t)in.n_users), omega, item_reg;
  if ((s = r.Read("LOSS", loss.data(), loss.size() * 4, err)) != kOk) return s;
  if (dual) {
    omega.resize((size_t)in.n_users);
    item_reg.resize((size_t)in.n_items);
    if ((s = r.Read("OMEGA", omega.data(), omega.size() * 4, err)) != kOk) return s;
    if ((s = r.Read("ITEMREG", item_reg.data(), item_reg.size() * 4, err)) != kOk) return s;
  }
  dm->RestoreVectors(loss.data(), dual ? omega.data() : nullptr, dual ? item_reg.data() : nullptr,
                     train);
  std::string text, e;
  if ((s = r.ReadText("STATE", &text, err)) != kOk) return s;
  KeyValues kv;
  if (!ParseKeyValues(text, &kv, &e) || !dm->RestoreState(kv, &e)) {
    if (err) *err = "STATE: " + e;
    return kInvalid;
  }
  if (train) dm->device().LoadTraining(*train);
  return kOk;
}

}  // namespace checkpoint
}  // namespace frecsys

#endif  // FRECSYS_CHECKPOINT_HOST_ONLY
