// checkpoint_check -- opens every file named on the command line with the
// host part of frecsys/checkpoint.h (full verification) and prints one line
// per file: "OK <path>", "INVALID <path>: <message>" or "IO <path>: <message>".
// A good file is also read section by section and written back to
// <path>.copy, which must verify and hold the same directory.  Built by
// tests/test_checkpoint_cpu.py with -fsanitize=address,undefined: malformed
// files must end as INVALID lines, not as sanitizer reports.
#define FRECSYS_CHECKPOINT_HOST_ONLY
#include <cstdio>
#include <string>
#include <vector>

#include "frecsys/checkpoint.h"

namespace ck = frecsys::checkpoint;

static bool rewrite(const ck::Reader& r, const std::string& path, std::string* err) {
  std::vector<std::pair<std::string, uint64_t>> lay;
  for (const ck::Section& s : r.sections()) lay.push_back({s.tag, s.bytes});
  ck::Writer w;
  if (w.Begin(path, r.info().flags, lay, err) != ck::kOk) return false;
  for (const ck::Section& s : r.sections()) {
    std::vector<unsigned char> buf((size_t)s.bytes);
    if (r.Read(s.tag, buf.data(), s.bytes, err) != ck::kOk) return false;
    if (w.Write(s.tag, buf.data(), s.bytes, err) != ck::kOk) return false;
  }
  if (w.Commit(err) != ck::kOk) return false;
  ck::Reader again;
  if (again.Open(path, true, err) != ck::kOk) return false;
  for (const ck::Section& s : r.sections()) {
    const ck::Section* t = again.Find(s.tag);
    if (!t || t->bytes != s.bytes || t->checksum != s.checksum) {
      *err = "section " + s.tag + " differs after the rewrite";
      return false;
    }
  }
  return true;
}

int main(int argc, char** argv) {
  int bad = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string path = argv[i];
    ck::Reader r;
    std::string err;
    const ck::Status s = r.Open(path, true, &err);
    if (s == ck::kInvalid) {
      printf("INVALID %s: %s\n", path.c_str(), err.c_str());
    } else if (s == ck::kIo) {
      printf("IO %s: %s\n", path.c_str(), err.c_str());
    } else if (!rewrite(r, path + ".copy", &err)) {
      printf("REWRITE-FAILED %s: %s\n", path.c_str(), err.c_str());
      bad = 1;
    } else {
      printf("OK %s\n", path.c_str());
    }
  }
  return bad;
}
