// Stand-alone check of csrc/p2p_wire.h (tests/test_p2p_wire.py builds it with ASan + UBSan and runs it):
// round trips, every strict prefix of a valid pull record, and each poisoned count.
#include <cstdio>
#include <cstdlib>

#include "../mpas-model_amd/csrc/p2p_wire.h"

using namespace p2p_wire;

#define REQUIRE(x)                                              \
  do {                                                          \
    if (!(x)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static Handle handle(char c) {
  Handle h;
  memset(h.bytes, c, sizeof(h.bytes));
  return h;
}

static bool same(const PullRecord& a, const PullRecord& b) {
  if (a.bufs.size() != b.bufs.size() || a.points.size() != b.points.size()) return false;
  for (size_t i = 0; i < a.bufs.size(); ++i)
    if (a.bufs[i].addr != b.bufs[i].addr || memcmp(&a.bufs[i].h, &b.bufs[i].h, sizeof(Handle))) return false;
  for (size_t p = 0; p < a.points.size(); ++p) {
    if (a.points[p].size() != b.points[p].size()) return false;
    for (size_t m = 0; m < a.points[p].size(); ++m) {
      const PullMsg &x = a.points[p][m], &y = b.points[p][m];
      if (x.dest != y.dest || x.segs.size() != y.segs.size()) return false;
      for (size_t k = 0; k < x.segs.size(); ++k) {
        const PullSeg &s = x.segs[k], &t = y.segs[k];
        if (s.buf != t.buf || s.off != t.off || s.n != t.n || s.inner != t.inner) return false;
        for (int i = 0; i < s.n; ++i)
          if (s.idx[i] != t.idx[i]) return false;  // read through the decoded pointer
      }
    }
  }
  return true;
}

// a record of one buffer, one exchange point, one message, one segment, written field by field:
// each count as given, `nlist` list values actually present
static std::vector<char> one(int32_t nbuf, int32_t npoint, int32_t nmsg, int32_t nseg, int32_t buf, int32_t n,
                             int nlist) {
  Writer w;
  w.put(nbuf);
  w.put((uint64_t)0x7f0000001000ull);
  w.put(handle('a'));
  w.put(npoint);
  w.put(nmsg);
  w.put((int32_t)1);  // dest
  w.put(nseg);
  w.put(buf);
  w.put((int64_t)4096);  // off
  w.put(n);
  w.put((int32_t)26);  // inner
  for (int i = 0; i < nlist; ++i) w.put((int32_t)(10 + i));
  return w.out;
}

int main() {
  PullRecord got;
  {  // empty
    const std::vector<char> b = PullRecord{}.encode();
    REQUIRE(PullRecord::decode(b.data(), b.size(), got));
    REQUIRE(got.bufs.empty() && got.points.empty());
  }
  // 2 buffers, 2 exchange points: a message with no segments, then one with n = 0 and n = 3
  const int32_t list[3] = {7, 0, 2561};
  PullRecord rec;
  rec.bufs = {{0x7f0000001000ull, handle('a')}, {0x7f0000200000ull, handle('b')}};
  rec.points.resize(2);
  rec.points[0].push_back(PullMsg{1, {}});
  rec.points[1].push_back(PullMsg{3, {PullSeg{1, 0, 0, 26, nullptr}, PullSeg{0, 8 * 2563, 3, 27, list}}});
  const std::vector<char> bytes = rec.encode();
  REQUIRE(PullRecord::decode(bytes.data(), bytes.size(), got));
  REQUIRE(same(rec, got));
  REQUIRE(got.points[1][0].segs[1].idx[2] == 2561);

  // every strict prefix fails (each in a buffer of its own size, so a read past it is seen)
  for (size_t len = 0; len < bytes.size(); ++len) {
    const std::vector<char> cut(bytes.begin(), bytes.begin() + len);
    REQUIRE(!PullRecord::decode(cut.data(), cut.size(), got));
  }
  {  // trailing bytes fail too
    std::vector<char> more(bytes);
    more.resize(bytes.size() + 4, 0);
    REQUIRE(!PullRecord::decode(more.data(), more.size(), got));
  }

  // poisoned counts; the field-by-field form is the encoder's when nothing is poisoned
  {
    const std::vector<char> ok = one(1, 1, 1, 1, 0, 3, 3);
    REQUIRE(PullRecord::decode(ok.data(), ok.size(), got));
    REQUIRE(ok == got.encode());
    REQUIRE(got.points[0][0].segs[0].idx[2] == 12);
    const std::vector<char> bad[] = {
        one(-1, 1, 1, 1, 0, 3, 3),  // buffer count
        one(1, -1, 1, 1, 0, 3, 3),  // exchange point count
        one(1, 1, -1, 1, 0, 3, 3),  // message count
        one(1, 1, 1, -1, 0, 3, 3),  // segment count
        one(1, 1, 1, 1, 0, -1, 3),  // n
        one(1, 1, 1, 1, 1, 3, 3),   // buffer id == table size
        one(1, 1, 1, 1, -1, 3, 3),  // buffer id < 0
        one(1, 1, 1, 1, 0, 4, 3),   // n one larger than the bytes that remain
        one(1, 1, 1, 1, 0, 0x7fffffff, 3),
    };
    for (const auto& b : bad) REQUIRE(!PullRecord::decode(b.data(), b.size(), got));
  }

  // the buffer record, 1 and 3 ranks, with a "no message" entry
  for (int nr : {1, 3}) {
    BufRecord br, out;
    br.points.resize(2);
    for (int i = 0; i < 2; ++i) {
      br.points[i].h = handle((char)('p' + i));
      for (int q = 0; q < nr; ++q) br.points[i].to.emplace_back(100 * i + q, 26 * (q + 1));
      br.points[i].to[nr - 1] = {-1, -1};
    }
    const std::vector<char> b = br.encode();
    REQUIRE(BufRecord::decode(b.data(), b.size(), out));
    REQUIRE(out.points.size() == 2);
    for (int i = 0; i < 2; ++i) {
      REQUIRE(!memcmp(&out.points[i].h, &br.points[i].h, sizeof(Handle)));
      REQUIRE(out.points[i].to == br.points[i].to);
    }
    for (size_t len = 0; len < b.size(); ++len) {
      const std::vector<char> cut(b.begin(), b.begin() + len);
      REQUIRE(!BufRecord::decode(cut.data(), cut.size(), out));
    }
  }
  {
    const std::vector<char> b = BufRecord{}.encode();
    BufRecord out;
    REQUIRE(BufRecord::decode(b.data(), b.size(), out) && out.points.empty());
    Writer w;
    w.put((int32_t)-1);
    REQUIRE(!BufRecord::decode(w.out.data(), w.out.size(), out));
    Writer v;
    v.put((int32_t)1);
    v.put(handle('x'));
    v.put((int32_t)-1);
    REQUIRE(!BufRecord::decode(v.out.data(), v.out.size(), out));
  }
  puts("p2p_wire: ok");
  return 0;
}
