"""MotionDetection::GetMotionsMaskHU (package_bgs/ck/MotionDetection.cpp:1256-1366) restated: background-rate map in, the class's
foreground mask, the cut labels and the flow value out.  Plain Python / numpy, one image at a time; the max-flow
is Dinic's on the cancelled terminal capacities, the labels are "reachable from the source in the residual graph"."""
from collections import deque

import numpy as np

SOURCE, SINK = 0, 1
DEFAULT_AREA, DEFAULT_WEIGHT = 5, 8.0


class Unsupported(ValueError):
    pass


def geometry(rows, cols, area=DEFAULT_AREA):
    """(NH, NW) of the node grid, or Unsupported for what bgs_lbpmrf_mask_check refuses"""
    if area < 3 or area % 2 == 0:
        raise Unsupported("histogram_area must be odd and at least 3")
    hw, nh = cols - area + 1, rows - area + 1
    if nh < 1 or hw < 2:
        raise Unsupported("the frame is smaller than the histogram area")
    if hw % 2:
        raise Unsupported("cols - histogram_area + 1 must be even")
    return nh, hw // 2


def sink_weights(rate, weight=DEFAULT_WEIGHT):
    """(short)(w * (1 - r)) in float arithmetic, truncated toward zero, clamped to [0, 32767]"""
    v = np.float32(weight) * (np.float32(1) - np.asarray(rate, np.float32))
    return np.clip(np.trunc(v.astype(np.float64)), 0, 32767).astype(np.int64)


def edges_of(nh, nw):
    """the reference's edges: node (x, y) to (x-1, y) and (x, y-1), only where x > 0 and y > 0"""
    out = []
    for y in range(1, nh):
        for x in range(1, nw):
            out.append((y * nw + x, y * nw + x - 1))
            out.append((y * nw + x, (y - 1) * nw + x))
    return out


def max_flow_labels(t, nh, nw, stats=None):
    """t: int [nh][nw] sink weights.  Returns (labels u8 [nh][nw], 1 = SINK, and the flow value Graph::maxflow() returns).
    stats["stranded"] counts the nodes that the source does not reach and that do not reach the sink either."""
    n = nh * nw
    S, T = n, n + 1
    to, cap, adj = [], [], [[] for _ in range(n + 2)]

    def add(u, v, cuv, cvu):
        adj[u].append(len(to)), to.append(v), cap.append(cuv)
        adj[v].append(len(to)), to.append(u), cap.append(cvu)

    tr = 1 - t.reshape(-1)  # set_tweights cancels the two capacities
    flow = int(np.minimum(1, t).sum())
    for u in range(n):
        if tr[u] > 0:
            add(S, u, int(tr[u]), 0)
        elif tr[u] < 0:
            add(u, T, int(-tr[u]), 0)
    for u, v in edges_of(nh, nw):
        add(u, v, 1, 1)
    while True:
        level = [-1] * (n + 2)
        level[S] = 0
        q = deque([S])
        while q:
            u = q.popleft()
            for e in adj[u]:
                if cap[e] > 0 and level[to[e]] < 0:
                    level[to[e]] = level[u] + 1
                    q.append(to[e])
        if level[T] < 0:
            break
        it = [0] * (n + 2)
        while True:  # one unit-or-more path at a time, iteratively
            path, u = [], S
            while u != T:
                while it[u] < len(adj[u]):
                    e = adj[u][it[u]]
                    if cap[e] > 0 and level[to[e]] == level[u] + 1:
                        break
                    it[u] += 1
                if it[u] == len(adj[u]):
                    if not path:
                        break
                    level[u] = -1  # dead end
                    u = to[path.pop() ^ 1]
                    continue
                path.append(adj[u][it[u]])
                u = to[path[-1]]
            if u != T:
                break
            f = min(cap[e] for e in path)
            for e in path:
                cap[e] -= f
                cap[e ^ 1] += f
            flow += f
    seen = [False] * (n + 2)  # the last BFS's levels are exactly the residual reachability from the source
    for u in range(n):
        seen[u] = level[u] >= 0
    labels = np.where(np.array(seen[:n]).reshape(nh, nw), SOURCE, SINK).astype(np.uint8)
    if stats is not None:
        reach = [False] * (n + 2)
        reach[T] = True
        q = deque([T])
        while q:
            w = q.popleft()
            for e in adj[w]:  # e is w -> x; x reaches w through the opposite arc
                if cap[e ^ 1] > 0 and not reach[to[e]]:
                    reach[to[e]] = True
                    q.append(to[e])
        stats["stranded"] += sum(1 for u in range(n) if not seen[u] and not reach[u])
    return labels, flow


def node_mask(labels, rows, cols, area=DEFAULT_AREA, stats=None):
    """:1322-1342: node pixels and the pixels in between, with the reference's own bounds tests"""
    nh, nw = labels.shape
    hw = 2 * nw
    sink = labels == SINK
    mask = np.zeros((rows, cols), np.uint8)
    for y in range(nh):
        for x in range(hw):
            if y % 2 == (x + 1) % 2:
                v = sink[y, x // 2]
                if stats is not None:
                    stats["node_255" if v else "node_0"] += 1
            else:
                tests = (x > 1, x < cols - area - 1, y > 0, y < rows - area)
                c = 0
                if tests[0]:
                    c += int(sink[y, x // 2 - 1])
                if tests[1]:
                    c += int(sink[y, x // 2 + 1])
                if tests[2]:
                    c += int(sink[y - 1, x // 2])
                if tests[3]:
                    c += int(sink[y + 1, x // 2])
                v = c > 1
                if stats is not None:
                    stats["between_255" if v else "between_0"] += 1
                    for k, name in enumerate(("left", "right", "up", "down")):
                        stats[name + "_bound_fails"] += not tests[k]
            mask[y + area - area // 2, x + area // 2] = 255 if v else 0
    return mask


def fill_holes(mask):
    """cvFloodFill from (0, 0) with 128, 4-connected, zero tolerances; then 128 -> 0 and 0 -> 255"""
    rows, cols = mask.shape
    m = mask.copy()
    seed = m[0, 0]
    reached = np.zeros((rows, cols), bool)
    reached[0, 0] = True
    q = deque([(0, 0)])
    while q:
        y, x = q.popleft()
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < rows and 0 <= xx < cols and not reached[yy, xx] and m[yy, xx] == seed:
                reached[yy, xx] = True
                q.append((yy, xx))
    m[reached] = 128
    out = m.copy()
    out[m == 128] = 0
    out[m == 0] = 255
    return out


def erode3(mask):
    """cvErode(src, dst, NULL, 1): the minimum over the 3 x 3 window, cells outside the image taking no part"""
    p = np.pad(mask, 1, constant_values=255)
    rows, cols = mask.shape
    out = np.full((rows, cols), 255, np.uint8)
    for dy in range(3):
        for dx in range(3):
            out = np.minimum(out, p[dy:dy + rows, dx:dx + cols])
    return out


def lbpmrf_mask(rate, rows, cols, area=DEFAULT_AREA, weight=DEFAULT_WEIGHT, stats=None):
    """rate: f32 [NH][NW].  Returns (mask u8 [rows][cols], labels u8 [NH][NW] with 1 = SINK, flow)."""
    nh, nw = geometry(rows, cols, area)
    rate = np.asarray(rate, np.float32)
    assert rate.shape == (nh, nw), (rate.shape, nh, nw)
    labels, flow = max_flow_labels(sink_weights(rate, weight), nh, nw, stats)
    return erode3(fill_holes(node_mask(labels, rows, cols, area, stats))), labels, flow


def duality(t, labels):
    """the capacity of the cut the labels describe: 1 per SINK node, t per SOURCE node, 1 per edge from a SOURCE to a SINK node (vectorised)"""
    src = labels == SOURCE
    cut = int((~src).sum()) + int(t[src].sum())
    cut += int((src[1:, 1:] != src[1:, :-1]).sum()) + int((src[1:, 1:] != src[:-1, 1:]).sum())
    return cut
