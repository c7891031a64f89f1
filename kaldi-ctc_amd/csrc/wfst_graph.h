// wfst_graph.h -- the decoding graph behind kctcGraph_t (include/kaldi_ctc_decode.h):
// a weighted finite-state transducer in the tropical semiring, validated and
// sorted on the host (wfst_graph.cpp; no HIP), and its device image, made by
// wfst_decode.hip at the first decode on a device.  Private to csrc/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

struct kctcGraphArc {
  int src, ilabel, olabel, dst;
  float weight;
};

struct kctcGraphImpl {
  typedef kctcGraphArc Arc;
  int num_states = 0, start = 0;
  std::vector<float> final_cost;    // [S], +inf: not final
  std::vector<Arc> arcs;            // stable-sorted by src: the position is the arc id
  std::vector<int> arc_off;         // [S + 1] CSR over arcs
  std::vector<int> ilabel_to_col;   // [max_ilabel + 1], entry 0 unused
  std::vector<int> eps_off, eps_arc;    // [S + 1], ids of the epsilon arcs of a state in arc order
  std::vector<int> emit_off, emit_arc;  // the same for the emitting arcs
  int eps_depth = 0;                // arcs on the longest epsilon path
  int max_ilabel = 0, max_col = -1; // max_col: highest column an emitting arc reads (-1: none)

  // device images, one per device (wfst_decode.hip makes and frees them)
  std::mutex dev_mutex;
  std::map<int, void *> dev;
  void (*dev_free)(int device, void *image) = nullptr;
  ~kctcGraphImpl();
};

namespace kctc {
namespace wfst {

typedef ::kctcGraphArc Arc;
typedef ::kctcGraphImpl Graph;

// Builds and validates; throws std::invalid_argument with the reason.
// ilabel_to_col: nullable (col(i) = i - 1), else num_ilabels entries indexed by ilabel.
Graph *make_graph(int num_states, int start, const float *final_costs, long num_arcs, const int *src,
                  const int *ilabel, const int *olabel, const float *weight, const int *dst,
                  const int *ilabel_to_col, int num_ilabels);
Graph *read_text(const std::string &path, const int *ilabel_to_col, int num_ilabels);
void write_text(const Graph &g, const std::string &path);

// number of words a path over T frames can emit at most, minus T: every frame
// is one emitting arc and between two of them lie at most eps_depth epsilon arcs
inline long words_slack(int eps_depth, int max_T) { return ((long)max_T + 1) * eps_depth; }

}  // namespace wfst
}  // namespace kctc
