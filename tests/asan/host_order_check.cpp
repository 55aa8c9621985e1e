// Sanitizer harness for the base row order of plan creation (msw_plan_create_ordered):
// tests/test_locality.py builds it with g++ -fsanitize=address,undefined and runs it.  It drives
// mswe-gnn_amd/csrc/graph_build.h build_host_graph with a row order on graphs and orders written by
// the test (the case layout of tests/asan/host_plan_check.cpp, each case followed by its order) and
// checks the numbering: with packing off, perm is the order with the padding inserted; with packing
// on, perm is tiling.h's pack_order applied to the in-degrees taken in that order; iperm inverts
// perm; a NULL order is the call without one; every bad order is refused with its position named.
//
//   host_order_check CASES.bin  ->  one JSON line per case on stdout
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "graph_build.h"

using namespace msw;

#define CHECK(cond, ...)                                              \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "CHECK failed (%s:%d): %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                              \
      std::fprintf(stderr, "\n");                                     \
      std::exit(3);                                                   \
    }                                                                 \
  } while (0)

struct Reader {
  FILE* f;
  int64_t i64() {
    int64_t v;
    CHECK(std::fread(&v, 8, 1, f) == 1, "truncated case file");
    return v;
  }
  std::vector<int64_t> vec(int64_t n) {
    CHECK(n >= 0 && n < (1LL << 32), "bad array length %lld", (long long)n);
    std::vector<int64_t> v((size_t)n);
    if (n) CHECK(std::fread(v.data(), 8, (size_t)n, f) == (size_t)n, "truncated array");
    return v;
  }
};

struct Case {
  std::string name;
  int64_t S, G, N, E, I;
  std::vector<int64_t> node_ptr, edge_index, edge_ptr, intra_index, intra_ptr, order;
};

static bool read_case(Reader& r, Case& c) {
  int64_t magic;
  if (std::fread(&magic, 8, 1, r.f) != 1) return false;
  CHECK(magic == 0x45534143, "bad case magic");
  const int64_t nlen = r.i64();
  std::vector<int64_t> nm = r.vec(nlen);
  c.name.assign(nm.begin(), nm.end());
  c.S = r.i64(); c.G = r.i64(); c.N = r.i64(); c.E = r.i64(); c.I = r.i64();
  (void)r.i64(); (void)r.i64(); (void)r.i64();  // expect_rc, group, rank: unused here
  c.node_ptr = r.vec(c.G * (c.S + 1));
  c.edge_index = r.vec(2 * c.E);
  c.edge_ptr = r.vec(c.S + 1);
  c.intra_index = r.vec(2 * c.I);
  c.intra_ptr = r.vec(c.S > 1 ? c.S : 0);
  CHECK(r.i64() == -1, "case %s carries an exchange", c.name.c_str());
  c.order = r.vec(c.N);
  return true;
}

static msw_graph_desc desc_of(const Case& c) {
  msw_graph_desc g{};
  g.num_nodes = c.N;
  g.num_scales = (int32_t)c.S;
  g.num_graphs = (int32_t)c.G;
  g.node_ptr = c.node_ptr.data();
  g.num_edges = c.E;
  g.edge_index = c.edge_index.data();
  g.edge_attr = nullptr;
  g.num_edge_features = 1;
  g.edge_ptr = c.edge_ptr.data();
  g.num_intra_edges = c.I;
  g.intra_edge_index = c.S > 1 ? c.intra_index.data() : nullptr;
  g.intra_edge_ptr = c.S > 1 ? c.intra_ptr.data() : nullptr;
  return g;
}

// perm as the header states it: scale-major, graph-major inside a scale, each range in `order`
// (through pack_order on the in-degrees taken in that order when `pack`), scale starts padded
static std::vector<int> expected_perm(const Case& c, const std::vector<int64_t>& order, int align, bool pack) {
  std::vector<int> indeg((size_t)c.N, 0);
  for (int64_t e = 0; e < c.E; ++e) ++indeg[(size_t)c.edge_index[c.E + e]];
  std::vector<int> perm;
  for (int s = 0; s < c.S; ++s) {
    for (int g = 0; g < c.G; ++g) {
      const int64_t a = c.node_ptr[g * (c.S + 1) + s], b = c.node_ptr[g * (c.S + 1) + s + 1];
      if (!pack) {
        for (int64_t v = a; v < b; ++v) perm.push_back((int)order[v]);
        continue;
      }
      std::vector<int> d((size_t)(b - a));
      for (int64_t v = a; v < b; ++v) d[v - a] = indeg[(size_t)order[v]];
      for (int k : pack_order(d)) perm.push_back((int)order[a + k]);
    }
    perm.resize((perm.size() + align - 1) / align * align, -1);
  }
  return perm;
}

static void check_numbering(const Case& c, const HostGraph& H, const std::vector<int>& want, const char* what) {
  CHECK(H.perm == want, "case %s (%s): perm is not the stated layout", c.name.c_str(), what);
  CHECK((int)H.iperm.size() == c.N, "iperm size");
  for (int i = 0; i < H.Npad; ++i)
    if (H.perm[i] >= 0) CHECK(H.iperm[H.perm[i]] == i, "perm / iperm not inverse at %d", i);
  for (int v = 0; v < c.N; ++v) CHECK(H.iperm[v] >= 0 && H.perm[H.iperm[v]] == v, "row %d unmapped", v);
}

// a bad order must be refused with MSW_ERR_INVALID and its first offending position named
static void expect_refusal(const Case& c, const msw_graph_desc& g, const std::vector<int64_t>& bad, int64_t pos,
                           const char* word) {
  HostGraph H;
  std::string err;
  for (int pack = 0; pack < 2; ++pack) {
    const int rc = build_host_graph(&g, (int)c.S, 64, pack != 0, 65536, H, err, bad.data());
    CHECK(rc == MSW_ERR_INVALID, "case %s: bad order (%s) gave rc %d", c.name.c_str(), word, rc);
    const std::string at = "row_order[" + std::to_string(pos) + "]";
    CHECK(err.find(at) != std::string::npos && err.find(word) != std::string::npos,
          "case %s: refusal '%s' does not name %s / '%s'", c.name.c_str(), err.c_str(), at.c_str(), word);
  }
}

int main(int argc, char** argv) {
  CHECK(argc == 2, "usage: host_order_check CASES.bin");
  Reader r{std::fopen(argv[1], "rb")};
  CHECK(r.f, "cannot open %s", argv[1]);
  std::vector<Case> cases;
  Case c;
  while (read_case(r, c)) cases.push_back(c);
  std::fclose(r.f);
  for (const Case& k : cases) {
    const msw_graph_desc g = desc_of(k);
    std::string err;
    std::vector<int64_t> ident((size_t)k.N);
    for (int64_t v = 0; v < k.N; ++v) ident[(size_t)v] = v;
    CHECK(k.order != ident, "case %s: the order is the identity and shows nothing", k.name.c_str());
    int moved = 0;
    for (int pack = 0; pack < 2; ++pack)
      for (int align : {16, 64}) {
        HostGraph H, H0, Hn;
        CHECK(build_host_graph(&g, (int)k.S, align, pack != 0, pack ? 65536 : 0, H, err, k.order.data()) == MSW_OK,
              "case %s: %s", k.name.c_str(), err.c_str());
        check_numbering(k, H, expected_perm(k, k.order, align, pack != 0), pack ? "packed" : "unpacked");
        // a NULL order is the call without one, and both are the identity order
        CHECK(build_host_graph(&g, (int)k.S, align, pack != 0, pack ? 65536 : 0, H0, err) == MSW_OK, "no order");
        CHECK(build_host_graph(&g, (int)k.S, align, pack != 0, pack ? 65536 : 0, Hn, err, nullptr) == MSW_OK, "NULL");
        CHECK(H0.perm == Hn.perm && H0.iperm == Hn.iperm, "case %s: NULL order differs from no order", k.name.c_str());
        check_numbering(k, H0, expected_perm(k, ident, align, pack != 0), "identity");
        moved += H.perm != H0.perm;
        // the plan's shape does not depend on the order
        CHECK(H.Npad == H0.Npad, "Npad");
        for (int s = 0; s < (int)k.S; ++s) CHECK(H.sc[s].n0 == H0.sc[s].n0 && H.sc[s].ns == H0.sc[s].ns, "scale rows");
      }
    CHECK(moved == 4, "case %s: the order did not take effect", k.name.c_str());

    // refusals: the first range with two rows, and a second range where there is one
    int64_t a0 = -1, b0 = -1, a1 = -1;
    for (int gi = 0; gi < k.G && a1 < 0; ++gi)
      for (int s = 0; s < k.S && a1 < 0; ++s) {
        const int64_t a = k.node_ptr[gi * (k.S + 1) + s], b = k.node_ptr[gi * (k.S + 1) + s + 1];
        if (b - a < 2) continue;
        if (a0 < 0) a0 = a, b0 = b;
        else a1 = a;
      }
    CHECK(a0 >= 0, "case %s has no range of two rows", k.name.c_str());
    int refusals = 0;
    {
      std::vector<int64_t> bad = k.order;  // a repeated entry: position a0 + 1 repeats a0's
      bad[(size_t)a0 + 1] = bad[(size_t)a0];
      expect_refusal(k, g, bad, a0 + 1, "repeats");
      ++refusals;
    }
    for (int64_t v : {(int64_t)-1, k.N, b0 == k.N ? a0 - 1 : b0}) {  // below 0, past N, just outside the range
      if (v >= a0 && v < b0) continue;
      std::vector<int64_t> bad = k.order;
      bad[(size_t)b0 - 1] = v;
      expect_refusal(k, g, bad, b0 - 1, "outside its range");
      ++refusals;
    }
    if (a1 >= 0) {  // two entries swapped across ranges (a scale or a graph): each range keeps its count
      std::vector<int64_t> bad = k.order;
      std::swap(bad[(size_t)a0], bad[(size_t)a1]);
      expect_refusal(k, g, bad, a0, "outside its range");  // ranges are checked in node_ptr's order
      ++refusals;
    }
    if (k.G > 1) {  // node_ptr ranges that overlap are named as such, not as a repeating order
      Case o = k;
      o.node_ptr[(size_t)(k.S + 1)] -= 1;  // the second graph starts on the first one's last row
      const msw_graph_desc go = desc_of(o);
      HostGraph H;
      const int rc = build_host_graph(&go, (int)k.S, 64, true, 65536, H, err, ident.data());
      CHECK(rc == MSW_ERR_INVALID && err == "node_ptr ranges overlap", "case %s: overlapping node_ptr gave rc %d (%s)",
            k.name.c_str(), rc, err.c_str());
      ++refusals;
    }
    std::printf("{\"case\": \"%s\", \"rows\": %lld, \"ranges_crossed\": %d, \"refusals\": %d}\n", k.name.c_str(),
                (long long)k.N, (int)(a1 >= 0), refusals);
  }
  return 0;
}
