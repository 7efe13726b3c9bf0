"""A sequential model of the data structures of MRP_LL_ASTAR_EPS_TA's device search (ll_ta.h runJobTaEps), for the
CPU tests: heap entries that CARRY their keys (focalH, f, g packed as in ll_device.h) instead of the reference's handles, a
position per node for the open AND the focal array, and the decrease-key of a_star_epsilon.hpp:254-269 done the way the
kernel does it — the open entry is re-keyed and sifted up, the focal entry is rewritten in place and nothing is sifted.
The heaps are boost's binary d_ary_heap (sift-up; sift-down preferring the first maximal child; erase = bubble to the root,
then pop) and the ordered walk's queue is libstdc++'s push_heap / pop_heap, both one element at a time.  If this model equals
the checker bit for bit, the kernel's representation loses nothing of the reference's handle-comparing focal heap."""
import struct

import ecbs_ta_corpus as cp

FH, FM, GM = 2047, 2047, 1023
def pack(fh, f, g, nid): return ((((FH - fh) << 21) | ((FM - f) << 10) | g), nid)
def kO(e): return e[0] & ((1 << 21) - 1)
def kF(e): return e[0]
def fOf(e): return FM - ((e[0] >> 10) & FM)
def gOf(e): return e[0] & GM
def fhOf(e): return FH - (e[0] >> 21)

def f32(x): return struct.unpack('f', struct.pack('f', x))[0]
def fmul(a, w): return f32(f32(float(a)) * f32(w))

class Heap:
    def __init__(s, key, nodes, posf): s.a = []; s.key = key; s.nodes = nodes; s.posf = posf
    def setpos(s, e, i):
        if s.posf: s.nodes[e[1]][s.posf] = i
    def sift_up(s, idx, e):
        a = s.a
        while idx > 0:
            p = (idx - 1) // 2
            if s.key(a[p]) < s.key(e):
                a[idx] = a[p]; s.setpos(a[p], idx); idx = p
            else: break
        a[idx] = e; s.setpos(e, idx)
    def push(s, e): s.a.append(None); s.sift_up(len(s.a) - 1, e)
    def sift_down(s, n, idx, x):
        a = s.a
        while True:
            c = 2 * idx + 1
            if c >= n: break
            if c + 1 < n and s.key(a[c]) < s.key(a[c + 1]): c += 1
            if s.key(a[c]) < s.key(x): break
            a[idx] = a[c]; s.setpos(a[c], idx); idx = c
        a[idx] = x; s.setpos(x, idx)
    def pop(s):
        last = s.a.pop()
        if s.a: s.sift_down(len(s.a), 0, last)
    def erase(s, pos):
        a = s.a
        while pos > 0:
            p = (pos - 1) // 2
            a[pos] = a[p]; s.setpos(a[p], pos); pos = p
        last = a.pop()
        if a: s.sift_down(len(a), 0, last)

def pq_push(a, v, key):
    a.append(v); hole = len(a) - 1
    while hole > 0:
        p = (hole - 1) // 2
        if key(a[p]) < key(v): a[hole] = a[p]; hole = p
        else: break
    a[hole] = v
def pq_pop(a, key):
    res = a[0]; value = a[-1]; a.pop(); ln = len(a)
    if ln == 0: return res
    hole = 0; sc = 0
    while sc < (ln - 1) // 2:
        sc = 2 * (sc + 1)
        if key(a[sc]) < key(a[sc - 1]): sc -= 1
        a[hole] = a[sc]; hole = sc
    if (ln & 1) == 0 and sc == (ln - 2) // 2:
        sc = 2 * (sc + 1); a[hole] = a[sc - 1]; hole = sc - 1
    while hole > 0:
        p = (hole - 1) // 2
        if key(a[p]) < key(value): a[hole] = a[p]; hole = p
        else: break
    a[hole] = value
    return res

def model(c):
    m = c["map"]; dimx, dimy = m["dimx"], m["dimy"]
    obst = {tuple(o) for o in m["obstacles"]}
    vcs = {tuple(v) for v in c["vc"]}; ecs = {tuple(e) for e in c["ec"]}
    goal = c["goal"]; w = c["w"]; agent = c["agent"]
    heur = cp.bfs_table(dimx, dimy, m["obstacles"], goal) if goal is not None else None
    last_goal = -1
    for t, x, y in vcs:
        if goal is None or [x, y] == list(goal): last_goal = max(last_goal, t)
    ctx = [p for i, p in enumerate(c["ctx"]) if i != agent and len(p) > 0]
    def at(p, t): return tuple(p[t]) if t < len(p) else tuple(p[-1])
    nodes = []
    openh = Heap(kO, nodes, "opos"); focal = Heap(kF, nodes, "fpos")
    sx, sy = c["start"]
    h0 = heur[sy][sx] if goal is not None else 0
    nodes.append(dict(x=sx, y=sy, t=0, parent=None, act=None, g=0, opos=0, fh=0, fpos=None))
    e0 = pack(0, h0, 0, 0); openh.push(e0); focal.push(e0)
    status = {(0, sx, sy): 1}
    bestF = h0; exp = 0; dk = 0
    while openh.a:
        top = openh.a[0]
        old = bestF; bestF = fOf(top)
        if bestF > old:
            lo, hi = fmul(old, w), fmul(bestF, w)
            aux = []; cur = (kO(openh.a[0]), 0)
            while True:
                i = cur[1]; first = 2 * i + 1
                if first < len(openh.a):
                    pq_push(aux, (kO(openh.a[first]), first), lambda v: v[0])
                    if first + 1 < len(openh.a): pq_push(aux, (kO(openh.a[first + 1]), first + 1), lambda v: v[0])
                fv = float(FM - ((cur[0] >> 10) & FM))
                if fv > lo and fv <= hi: focal.push(openh.a[i])
                if fv > hi: break
                if not aux: break
                cur = pq_pop(aux, lambda v: v[0])
        cur = focal.a[0]; cid = cur[1]; gcur = gOf(cur); cfh = fhOf(cur)
        nd = nodes[cid]; x, y, t = nd["x"], nd["y"], nd["t"]
        exp += 1
        if c["cap"] >= 0 and exp > c["cap"]: return dict(rc=-1, expanded=exp)
        at_goal = goal is None or [x, y] == list(goal)
        if at_goal and t > last_goal:
            st = []; k = cid
            while k is not None: st.append([nodes[k]["t"], nodes[k]["x"], nodes[k]["y"]]); k = nodes[k]["parent"]
            return dict(rc=0, success=True, cost=gcur, fmin=fOf(top), expanded=exp, states=st[::-1], dk=dk)
        focal.pop(); openh.erase(nd["opos"]); status[(t, x, y)] = -1
        bound = fmul(bestF, w)
        for k, (dx, dy) in enumerate([(0, 0), (-1, 0), (1, 0), (0, 1), (0, -1)]):
            nx, ny, t1 = x + dx, y + dy, t + 1
            if not (0 <= nx < dimx and 0 <= ny < dimy) or (nx, ny) in obst or (t1, nx, ny) in vcs: continue
            if (t, x, y, nx, ny) in ecs: continue
            st = status.get((t1, nx, ny), 0)
            if st == -1: continue
            g2 = gcur + (0 if (k == 0 and at_goal) else 1)
            if st == 0:
                h = heur[ny][nx] if goal is not None else 0
                cnt = 0
                for p in ctx:
                    a, b = at(p, t), at(p, t1)
                    if b == (nx, ny): cnt += 1
                    if a == (nx, ny) and b == (x, y): cnt += 1
                nid = len(nodes)
                nodes.append(dict(x=nx, y=ny, t=t1, parent=cid, act=k, g=g2, opos=0, fh=cfh + cnt, fpos=None))
                status[(t1, nx, ny)] = nid + 1
                e = pack(cfh + cnt, g2 + h, g2, nid)
                openh.push(e)
                if float(g2 + h) <= bound: focal.push(e)
            else:
                nid = st - 1; on = nodes[nid]
                if g2 >= on["g"]: continue
                dk += 1
                fold = fOf(openh.a[on["opos"]]); fnew = fold - (on["g"] - g2)
                on["g"] = g2; on["parent"] = cid; on["act"] = k
                e = pack(on["fh"], fnew, g2, nid)
                openh.sift_up(on["opos"], e)
                if on["fpos"] is not None: focal.a[on["fpos"]] = e
                elif float(fnew) <= bound and float(fold) > bound: focal.push(e)
    return dict(rc=0, success=False, expanded=exp)
