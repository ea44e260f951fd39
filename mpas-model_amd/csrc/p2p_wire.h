// The records the ranks all-gather to set up the one-sided halo transfer (p2p_setup.hip): what the
// bytes of a record are, and nothing else.  Plain C++17 with no HIP include, so the code that
// parses another process's bytes builds and runs on a CPU under sanitizers (tests/p2p_wire_check.cpp).
//
// Every value is written with memcpy at its own size, so the layout does not depend on struct
// padding; every size is a multiple of 4, so a send list inside 4-byte-aligned bytes is aligned.
// decode() returns false on any malformed input (truncated, trailing bytes, a negative count, a
// buffer id outside the table, a list that runs past the end); the caller then uses none of `out`.
#pragma once
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace p2p_wire {

struct Handle {  // opaque: a hipIpcMemHandle_t (p2p_setup.hip asserts the size)
  char bytes[64];
};

struct Writer {
  std::vector<char> out;
  void put_bytes(const void* v, size_t n) {
    if (n) out.insert(out.end(), (const char*)v, (const char*)v + n);
  }
  template <class T, class... More>
  void put(const T& v, const More&... more) {
    static_assert(sizeof(T) % 4 == 0, "records keep 4-byte alignment");
    put_bytes(&v, sizeof(T));
    if constexpr (sizeof...(More) > 0) put(more...);
  }
};

struct Reader {  // never reads at or past `end`
  const char *p, *end;
  bool has(size_t n) const { return (size_t)(end - p) >= n; }
  template <class T, class... More>
  bool get(T& v, More&... more) {
    if (!has(sizeof(T))) return false;
    memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    if constexpr (sizeof...(More) > 0) return get(more...);
    return true;
  }
  bool get_count(int32_t& n) { return get(n) && n >= 0; }
  // n int32 values in place: a pointer into the bytes read, refused unless aligned
  bool get_list(int32_t n, const int32_t*& v) {
    if (n < 0 || !has(4 * (size_t)n) || (uintptr_t)p % alignof(int32_t)) return false;
    v = (const int32_t*)p;
    p += 4 * (size_t)n;
    return true;
  }
};

// ---- the pull record: a rank's exported field buffers and, per exchange point, its messages ----
struct PullBuf {
  uint64_t addr;  // in the exporting process
  Handle h;
};
struct PullSeg {       // one pack segment
  int32_t buf;         // index into PullRecord::bufs
  int64_t off;         // bytes from the buffer's start
  int32_t n, inner;    // columns, doubles per column
  const int32_t* idx;  // the send list, n entries (decoded: points into the bytes decoded)
};
struct PullMsg {
  int32_t dest;               // destination rank
  std::vector<PullSeg> segs;  // in buffer order
};
struct PullRecord {
  std::vector<PullBuf> bufs;
  std::vector<std::vector<PullMsg>> points;  // per exchange point
  bool fits(size_t npoints, int) const { return points.size() == npoints; }

  std::vector<char> encode() const {
    Writer w;
    w.put((int32_t)bufs.size());
    for (const PullBuf& b : bufs) w.put(b.addr, b.h);
    w.put((int32_t)points.size());
    for (const auto& msgs : points) {
      w.put((int32_t)msgs.size());
      for (const PullMsg& m : msgs) {
        w.put(m.dest, (int32_t)m.segs.size());
        for (const PullSeg& s : m.segs) {
          w.put(s.buf, s.off, s.n, s.inner);
          w.put_bytes(s.idx, 4 * (size_t)s.n);
        }
      }
    }
    return std::move(w.out);
  }

  // `data` must outlive `out` (the send lists point into it)
  static bool decode(const char* data, size_t len, PullRecord& out) {
    Reader r{data, data + len};
    out = PullRecord{};
    int32_t nbuf, npoint, nmsg, nseg;
    if (!r.get_count(nbuf)) return false;
    for (int32_t i = 0; i < nbuf; ++i) {
      PullBuf b;
      if (!r.get(b.addr, b.h)) return false;
      out.bufs.push_back(b);
    }
    if (!r.get_count(npoint)) return false;
    for (int32_t i = 0; i < npoint; ++i) {
      if (!r.get_count(nmsg)) return false;
      out.points.emplace_back();
      for (int32_t m = 0; m < nmsg; ++m) {
        PullMsg msg;
        if (!r.get(msg.dest) || !r.get_count(nseg)) return false;
        for (int32_t k = 0; k < nseg; ++k) {
          PullSeg s;
          if (!r.get(s.buf, s.off, s.n, s.inner) || !r.get_list(s.n, s.idx) || s.buf < 0 || s.buf >= nbuf) return false;
          msg.segs.push_back(s);
        }
        out.points.back().push_back(std::move(msg));
      }
    }
    return r.p == r.end;
  }
};

// ---- the buffer record: per exchange point, the send buffer and where each rank's message lies ----
struct BufPoint {
  Handle h;                                     // the send buffer
  std::vector<std::pair<int64_t, int64_t>> to;  // by rank: (offset, count) in doubles, (-1, -1) no message
};
struct BufRecord {
  std::vector<BufPoint> points;
  bool fits(size_t npoints, int nranks) const {
    for (const BufPoint& p : points)
      if (p.to.size() != (size_t)nranks) return false;
    return points.size() == npoints;
  }

  std::vector<char> encode() const {
    Writer w;
    w.put((int32_t)points.size());
    for (const BufPoint& p : points) {
      w.put(p.h, (int32_t)p.to.size());
      for (const auto& oc : p.to) w.put(oc.first, oc.second);
    }
    return std::move(w.out);
  }

  static bool decode(const char* data, size_t len, BufRecord& out) {
    Reader r{data, data + len};
    out = BufRecord{};
    int32_t npoint, nrank;
    if (!r.get_count(npoint)) return false;
    for (int32_t i = 0; i < npoint; ++i) {
      BufPoint p;
      if (!r.get(p.h) || !r.get_count(nrank)) return false;
      for (int32_t q = 0; q < nrank; ++q) {
        p.to.emplace_back();
        if (!r.get(p.to.back().first, p.to.back().second)) return false;
      }
      out.points.push_back(std::move(p));
    }
    return r.p == r.end;
  }
};

}  // namespace p2p_wire
