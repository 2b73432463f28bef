// Grouping of the classifier's in-place 180-degree rotations (cv::rotate on ROI views that alias their image): only ROIs
// that intersect constrain each other.  The ROIs of a view (the key: whatever identifies the image a rectangle lies in;
// different views do not alias) are grouped into the connected components of "intersects"; a component keeps request order
// and is applied by one workgroup of rotate180_groups_kernel, components run concurrently.  Host arithmetic only - no HIP,
// no device types - so that ocr_selftest_rotation_groups hands out exactly what rotate180_in_order (pipe.hip) launches.
#pragma once
#include <algorithm>
#include <map>
#include <vector>

namespace ocr {
namespace rot_groups {

struct Rect { int x, y, w, h; };

inline bool intersects(const Rect& e, const Rect& q) {
  return e.x < q.x + q.w && q.x < e.x + e.w && e.y < q.y + q.h && q.y < e.y + e.h;
}

// order: the n request indices, group after group, groups in order of their first ROI, members in request order;
// seg: ngroups + 1 offsets into order
template <class Key>
inline void group(const std::vector<Rect>& rects, const std::vector<Key>& view, std::vector<int>& order, std::vector<int>& seg) {
  const int n = (int)rects.size();
  std::vector<int> parent(n);
  for (int i = 0; i < n; ++i) parent[i] = i;
  auto find = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
  std::map<Key, std::vector<int>> views;  // per view the list is short (the lines of one image)
  for (int k = 0; k < n; ++k) {
    std::vector<int>& mine = views[view[k]];
    for (int j : mine) {
      if (intersects(rects[j], rects[k])) {
        const int a = find(j), b = find(k);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);  // the root is the component's first ROI
      }
    }
    mine.push_back(k);
  }
  std::vector<std::vector<int>> members(n);
  for (int k = 0; k < n; ++k) members[find(k)].push_back(k);
  order.clear();
  order.reserve(n);
  seg.assign(1, 0);
  for (int r = 0; r < n; ++r) {
    if (members[r].empty()) continue;
    for (int k : members[r]) order.push_back(k);
    seg.push_back((int)order.size());
  }
}

}  // namespace rot_groups
}  // namespace ocr
