// wfst_graph.cpp -- the host side of decoding graphs (include/kaldi_ctc_decode.h,
// DESIGN.md §7g): the graph object, its validation, the arc sort and the CSR
// views, eps_depth, and the OpenFst text form.  Nothing here touches the GPU;
// the device image is made by wfst_decode.hip at the first decode.
#include "wfst_graph.h"

#include <algorithm>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <numeric>
#include <sstream>
#include <stdexcept>

#include "kaldi_ctc_decode.h"

// kctc_last_error() text of the calling thread (nnet_api.cpp)
void kctc_set_error(const char *msg);

// runs f, mapping exceptions to a non-zero return and kctc_last_error(); the
// copy of nnet_handle.h's kctc_guarded that keeps this file free of HIP headers
template <typename F>
static int guarded(F f) {
  try {
    f();
    return 0;
  } catch (const std::exception &e) {
    kctc_set_error(e.what());
    return 1;
  } catch (...) {
    kctc_set_error("unknown error");
    return 1;
  }
}
#define GRAPH_REQUIRE(cond, msg)                               \
  do {                                                         \
    if (!(cond)) throw std::invalid_argument(std::string(msg)); \
  } while (0)

kctcGraphImpl::~kctcGraphImpl() {
  if (dev_free)
    for (auto &kv : dev) dev_free(kv.first, kv.second);
}

namespace kctc {
namespace wfst {

static void fail(const std::string &msg) { throw std::invalid_argument("graph: " + msg); }

Graph *make_graph(int S, int start, const float *final_costs, long num_arcs, const int *src, const int *ilabel,
                  const int *olabel, const float *weight, const int *dst, const int *ilabel_to_col,
                  int num_ilabels) {
  if (S < 1) fail("no states");
  if (start < 0 || start >= S) fail("start state out of range");
  if (!final_costs) fail("null final costs");
  if (num_arcs < 0 || num_arcs > INT_MAX - 2) fail("arc count out of range");
  if (num_arcs > 0 && (!src || !ilabel || !olabel || !weight || !dst)) fail("null arc array");
  if (ilabel_to_col && num_ilabels < 1) fail("empty ilabel_to_col");
  for (int s = 0; s < S; s++) {
    const float f = final_costs[s];
    if (std::isnan(f) || f == -INFINITY) fail("final cost of state " + std::to_string(s) + " is NaN or -inf");
  }
  int max_il = 0;
  for (long a = 0; a < num_arcs; a++) {
    const std::string at = " of arc " + std::to_string(a);
    if (src[a] < 0 || src[a] >= S) fail("source state" + at + " out of range");
    if (dst[a] < 0 || dst[a] >= S) fail("destination state" + at + " out of range");
    if (ilabel[a] < 0) fail("negative ilabel" + at);
    if (olabel[a] < 0) fail("negative olabel" + at);
    if (ilabel_to_col && ilabel[a] >= num_ilabels) fail("ilabel" + at + " outside ilabel_to_col");
    if (!std::isfinite(weight[a])) fail("weight" + at + " is not finite");
    max_il = std::max(max_il, ilabel[a]);
  }
  std::unique_ptr<Graph> g(new Graph);
  g->num_states = S;
  g->start = start;
  g->final_cost.assign(final_costs, final_costs + S);
  g->max_ilabel = max_il;
  g->ilabel_to_col.assign((size_t)max_il + 1, -1);
  for (int i = 1; i <= max_il; i++) g->ilabel_to_col[i] = ilabel_to_col ? ilabel_to_col[i] : i - 1;
  // arc ids: positions after a stable sort by source state
  std::vector<int> order((size_t)num_arcs);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return src[a] < src[b]; });
  g->arcs.resize((size_t)num_arcs);
  g->arc_off.assign((size_t)S + 1, 0);
  g->eps_off.assign((size_t)S + 1, 0);
  g->emit_off.assign((size_t)S + 1, 0);
  for (long k = 0; k < num_arcs; k++) {
    const int a = order[k];
    g->arcs[k] = Arc{src[a], ilabel[a], olabel[a], dst[a], weight[a]};
    g->arc_off[src[a] + 1]++;
    if (ilabel[a] == 0) {
      g->eps_off[src[a] + 1]++;
    } else {
      g->emit_off[src[a] + 1]++;
      const int c = g->ilabel_to_col[ilabel[a]];
      if (c < 0) fail("column of ilabel " + std::to_string(ilabel[a]) + " is negative");
      g->max_col = std::max(g->max_col, c);
    }
  }
  for (int s = 0; s < S; s++) {
    g->arc_off[s + 1] += g->arc_off[s];
    g->eps_off[s + 1] += g->eps_off[s];
    g->emit_off[s + 1] += g->emit_off[s];
  }
  g->eps_arc.reserve(g->eps_off[S]);
  g->emit_arc.reserve(g->emit_off[S]);
  for (long k = 0; k < num_arcs; k++) (g->arcs[k].ilabel == 0 ? g->eps_arc : g->emit_arc).push_back((int)k);
  // eps_depth: the longest path of the epsilon subgraph, in topological order
  // (Kahn); states left over sit on or behind a cycle
  std::vector<int> indeg((size_t)S, 0), depth((size_t)S, 0), queue;
  for (int k : g->eps_arc) indeg[g->arcs[k].dst]++;
  for (int s = 0; s < S; s++)
    if (indeg[s] == 0) queue.push_back(s);
  for (size_t q = 0; q < queue.size(); q++) {
    const int s = queue[q];
    for (int e = g->eps_off[s]; e < g->eps_off[s + 1]; e++) {
      const int d = g->arcs[g->eps_arc[e]].dst;
      depth[d] = std::max(depth[d], depth[s] + 1);
      g->eps_depth = std::max(g->eps_depth, depth[d]);
      if (--indeg[d] == 0) queue.push_back(d);
    }
  }
  if ((int)queue.size() != S) fail("the epsilon arcs form a cycle");
  return g.release();
}

static long parse_int(const std::string &tok, const std::string &path, long line) {
  errno = 0;
  char *end = nullptr;
  const long v = std::strtol(tok.c_str(), &end, 10);
  if (tok.empty() || *end || errno || v < 0 || v > INT_MAX)
    fail(path + ":" + std::to_string(line) + ": '" + tok + "' is not a non-negative integer (symbol tables are not read)");
  return v;
}
static float parse_weight(const std::string &tok, const std::string &path, long line) {
  char *end = nullptr;
  const float v = std::strtof(tok.c_str(), &end);
  if (tok.empty() || *end) fail(path + ":" + std::to_string(line) + ": '" + tok + "' is not a weight");
  return v;
}

Graph *read_text(const std::string &path, const int *ilabel_to_col, int num_ilabels) {
  std::ifstream is(path);
  if (!is) throw std::runtime_error("cannot read graph " + path);
  std::vector<int> src, il, ol, dst;
  std::vector<float> w;
  std::vector<std::pair<int, float>> finals;
  int start = -1, max_state = -1;
  std::string text;
  long line = 0;
  while (std::getline(is, text)) {
    line++;
    std::istringstream ls(text);
    std::vector<std::string> tok;
    for (std::string t; ls >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    const int s = (int)parse_int(tok[0], path, line);
    if (start < 0) start = s;
    max_state = std::max(max_state, s);
    if (tok.size() <= 2) {  // state [weight]
      finals.emplace_back(s, tok.size() == 2 ? parse_weight(tok[1], path, line) : 0.f);
    } else if (tok.size() == 4 || tok.size() == 5) {  // src dst ilabel olabel [weight]
      src.push_back(s);
      dst.push_back((int)parse_int(tok[1], path, line));
      il.push_back((int)parse_int(tok[2], path, line));
      ol.push_back((int)parse_int(tok[3], path, line));
      w.push_back(tok.size() == 5 ? parse_weight(tok[4], path, line) : 0.f);
      max_state = std::max(max_state, dst.back());
    } else {
      fail(path + ":" + std::to_string(line) + ": expected 1, 2, 4 or 5 fields");
    }
  }
  if (start < 0) fail(path + ": empty graph");
  std::vector<float> fin((size_t)max_state + 1, INFINITY);
  for (auto &f : finals) fin[f.first] = f.second;
  return make_graph(max_state + 1, start, fin.data(), (long)src.size(), src.data(), il.data(), ol.data(), w.data(),
                    dst.data(), ilabel_to_col, num_ilabels);
}

void write_text(const Graph &g, const std::string &path) {
  std::ofstream os(path, std::ios::trunc);
  if (!os) throw std::runtime_error("cannot write graph " + path);
  os.precision(9);  // a float survives the round trip
  // the start state is the source of the first line: its arcs (or its final line) go first
  auto state = [&](int s) {
    for (int k = g.arc_off[s]; k < g.arc_off[s + 1]; k++) {
      const Arc &a = g.arcs[k];
      os << a.src << ' ' << a.dst << ' ' << a.ilabel << ' ' << a.olabel << ' ' << a.weight << '\n';
    }
    if (g.final_cost[s] != INFINITY) os << s << ' ' << g.final_cost[s] << '\n';
  };
  state(g.start);
  if (g.arc_off[g.start] == g.arc_off[g.start + 1] && g.final_cost[g.start] == INFINITY)
    os << g.start << " Infinity\n";  // a start state without arcs and not final still names itself
  for (int s = 0; s < g.num_states; s++)
    if (s != g.start) state(s);
  // a highest state that no line mentions would shrink the graph on reading
  const int last = g.num_states - 1;
  if (last != g.start && g.arc_off[last] == g.arc_off[last + 1] && g.final_cost[last] == INFINITY) {
    bool seen = false;
    for (const Arc &a : g.arcs) seen = seen || a.dst == last;
    if (!seen) os << last << " Infinity\n";
  }
  os.flush();
  if (!os) throw std::runtime_error("error writing graph " + path);
}

}  // namespace wfst
}  // namespace kctc

extern "C" {

int kctc_graph_create(kctcGraph_t *graph, int num_states, int start, const float *final_costs, long num_arcs,
                      const int *src, const int *ilabel, const int *olabel, const float *weight, const int *dst,
                      const int *ilabel_to_col, int num_ilabels) {
  return guarded([&] {
    GRAPH_REQUIRE(graph, "kctc_graph_create: null argument");
    *graph = kctc::wfst::make_graph(num_states, start, final_costs, num_arcs, src, ilabel, olabel, weight, dst,
                                    ilabel_to_col, num_ilabels);
  });
}

int kctc_graph_read_text(kctcGraph_t *graph, const char *path, const int *ilabel_to_col, int num_ilabels) {
  return guarded([&] {
    GRAPH_REQUIRE(graph && path, "kctc_graph_read_text: null argument");
    *graph = kctc::wfst::read_text(path, ilabel_to_col, num_ilabels);
  });
}

int kctc_graph_write_text(kctcGraph_t graph, const char *path) {
  return guarded([&] {
    GRAPH_REQUIRE(graph && path, "kctc_graph_write_text: null argument");
    kctc::wfst::write_text(*graph, path);
  });
}

int kctc_graph_info(kctcGraph_t graph, int *num_states, long *num_arcs, int *eps_depth, int *max_ilabel,
                    int *max_col) {
  return guarded([&] {
    GRAPH_REQUIRE(graph, "kctc_graph_info: null argument");
    if (num_states) *num_states = graph->num_states;
    if (num_arcs) *num_arcs = (long)graph->arcs.size();
    if (eps_depth) *eps_depth = graph->eps_depth;
    if (max_ilabel) *max_ilabel = graph->max_ilabel;
    if (max_col) *max_col = graph->max_col;
  });
}

int kctc_graph_get(kctcGraph_t graph, int *start, float *final_costs, int *src, int *ilabel, int *olabel,
                   float *weight, int *dst) {
  return guarded([&] {
    GRAPH_REQUIRE(graph, "kctc_graph_get: null argument");
    if (start) *start = graph->start;
    if (final_costs) std::copy(graph->final_cost.begin(), graph->final_cost.end(), final_costs);
    for (size_t k = 0; k < graph->arcs.size(); k++) {
      const kctcGraphArc &a = graph->arcs[k];
      if (src) src[k] = a.src;
      if (ilabel) ilabel[k] = a.ilabel;
      if (olabel) olabel[k] = a.olabel;
      if (weight) weight[k] = a.weight;
      if (dst) dst[k] = a.dst;
    }
  });
}

int kctc_graph_destroy(kctcGraph_t graph) {
  return guarded([&] { delete graph; });
}

}  // extern "C"
