// Per-node records of the exact KNN's implicit Morton octree (knn.hip): for every node of every level its range in the sorted point array and the exact
// fp32 bounding box of the points in that range.  The search prunes by this box, not by the node's cell: a sparse node's points fill a small part of its cell.
//
// Index: heap order.  The root is node 0; the children of node i are 8 i + 1 .. 8 i + 8, so the node of depth d (level GRID_BITS - d) with Morton prefix m is
// (8^d - 1) / 7 + m and a child's record is found from its parent's index alone.  Depth 6 holds the 64^3 fine cells.
// Built bottom-up once per frame: depth 6 from the sorted points, every depth above as the min / max / sum over its 8 children (deterministic: no atomics).
//
// The bodies are host-and-device functions so that tests/test_knn_node_records.py can run exactly this code on the CPU (it compiles this header alone).
#pragma once

#if defined(__HIPCC__)
#define NL_NODE_FN __host__ __device__ inline
#else
#define NL_NODE_FN inline
#endif

constexpr int NL_KNN_DEPTH = 6;                                  // = GRID_BITS: 64 fine cells per axis
constexpr int NL_KNN_NODES = ((1 << (3 * (NL_KNN_DEPTH + 1))) - 1) / 7;   // 8^0 + ... + 8^6 = 299593

struct alignas(16) NlKnnNode {   // two 16-byte halves
  int start, count;              // the node's points are sorted[start .. start + count)
  float mnx, mny;
  float mnz, mxx, mxy, mxz;      // count == 0: min = +3.4e38, max = -3.4e38 (the identity of the reduction; the search tests count first)
};

NL_NODE_FN int nl_knn_node_base(int depth) { return ((1 << (3 * depth)) - 1) / 7; }

// depth-6 record of fine cell `cell` (its Morton code); sorted4: x, y, z, index bits per point
NL_NODE_FN void nl_knn_node_from_points(NlKnnNode* nodes, const int* starts, const float* sorted4, int cell) {
  NlKnnNode r;
  r.start = starts[cell];
  r.count = starts[cell + 1] - r.start;
  r.mnx = r.mny = r.mnz = 3.4e38f;
  r.mxx = r.mxy = r.mxz = -3.4e38f;
  for (int i = 0; i < r.count; ++i) {
    const float* p = sorted4 + 4 * (long long)(r.start + i);
    r.mnx = p[0] < r.mnx ? p[0] : r.mnx; r.mxx = p[0] > r.mxx ? p[0] : r.mxx;
    r.mny = p[1] < r.mny ? p[1] : r.mny; r.mxy = p[1] > r.mxy ? p[1] : r.mxy;
    r.mnz = p[2] < r.mnz ? p[2] : r.mnz; r.mxz = p[2] > r.mxz ? p[2] : r.mxz;
  }
  nodes[nl_knn_node_base(NL_KNN_DEPTH) + cell] = r;
}

// record of node i (depth < 6) from its 8 children, which are contiguous in the sorted array in child order
NL_NODE_FN void nl_knn_node_from_children(NlKnnNode* nodes, int i) {
  const NlKnnNode* ch = nodes + 8 * (long long)i + 1;
  NlKnnNode r = ch[0];
  for (int k = 1; k < 8; ++k) {
    const NlKnnNode c = ch[k];
    r.count += c.count;
    r.mnx = c.mnx < r.mnx ? c.mnx : r.mnx; r.mxx = c.mxx > r.mxx ? c.mxx : r.mxx;
    r.mny = c.mny < r.mny ? c.mny : r.mny; r.mxy = c.mxy > r.mxy ? c.mxy : r.mxy;
    r.mnz = c.mnz < r.mnz ? c.mnz : r.mnz; r.mxz = c.mxz > r.mxz ? c.mxz : r.mxz;
  }
  nodes[i] = r;
}
