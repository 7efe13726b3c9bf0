// The arena tier's building blocks: what every search that keeps its state in the arena slot is made of.
//   * DEVI, the DBG / PROF macros of the diagnostic builds, lane helpers (ballot64, rfl, waveShr1);
//   * the tiers: TierHbm (64-bit heap entries, four-word node records in global memory) and the variants derived from it
//     — TierHyb / TierHybXy (heap tops in LDS: the CBS / ECBS arena search), TierFocalPos (runJobTaEps); SIPP's own
//     tiers are in ll_sipp.h;
//   * Mem<T>, one search's arrays seen through a tier's types, viewAs, Ctx and SState;
//   * the exact array-heap emulations: siftUp, descend, heapPop, PushChains, popFocalEraseOpen, and the ordered walk.
// Needs ll_device.h (key field widths, DevResult).  Included by ll_kernel.hip only, first of the arena-tier headers.
#ifndef MRP_LL_ARENA_HEAP_H
#define MRP_LL_ARENA_HEAP_H

namespace mrp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

#define DEVI __device__ __forceinline__

#ifdef MRP_LL_TRACE  // diagnostic build only (-DMRP_LL_TRACE): progress words in a host-mapped buffer
#define DBG(P, slot, val)                                                                      \
  do {                                                                                         \
    if ((P).debug && blockIdx.x < 4096) { /* all lanes store the same word */                  \
      (P).debug[blockIdx.x * 16 + (slot)] = (uint32_t)(val);                                   \
      __threadfence_system();                                                                  \
    }                                                                                          \
  } while (0)
#define PROF_T0() uint64_t prof_t0__ = __builtin_amdgcn_s_memtime()
#define PROF_ADD(res, k) (res).prof[k] += (uint32_t)(__builtin_amdgcn_s_memtime() - prof_t0__)
#define PROF_INC(res, k, v) (res).prof[k] += (uint32_t)(v)
#define PROF_MARK(var) uint64_t var = __builtin_amdgcn_s_memtime()
#define PROF_SINCE(res, k, var) (res).prof[k] += (uint32_t)(__builtin_amdgcn_s_memtime() - var)
#else
#define DBG(P, slot, val) do { } while (0)
#define PROF_MARK(var) do { } while (0)
#define PROF_SINCE(res, k, var) do { } while (0)
#define PROF_T0() do { } while (0)
#define PROF_ADD(res, k) do { } while (0)
#define PROF_INC(res, k, v) do { } while (0)
#endif

DEVI uint64_t ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }  // no bool -> int -> bool round trip
DEVI uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
DEVI int32_t rfli(int32_t v) { return (int32_t)__builtin_amdgcn_readfirstlane((uint32_t)v); }
DEVI uint64_t rfl64(uint64_t v) {
  uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

DEVI uint32_t waveShr1(uint32_t v) {  // lane i receives lane i-1's value (lane 0 keeps its own)
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false);
}

// ---- memory tiers and their record formats ---------------------------------------------------------------------
// A heap entry carries its sort key and the node id.  A larger key is a BETTER node in the reference's orders:
//   open  (a_star_epsilon.hpp:312-323, a_star.hpp:168-179): lowest f, then highest g      -> keyOpen
//   focal (a_star_epsilon.hpp:346-366): lowest focalH, then lowest f, then highest g      -> keyFocal
// Entries with equal keys compare EQUAL (the id never takes part), exactly like the reference's comparators; which of
// two equal entries comes out first is decided by the heap layout, which the kernels replay verbatim.
//
// TierHbm (global memory, the search's arena slot; also what SIPP uses): 64-bit entries as laid out in ll_device.h,
//   16-byte node records {x | y<<8 | t<<16 | action<<27, parent id, focalH, position in the open array}.
//   (The CBS / ECBS fast tier is ll_compact.h: its 32-bit entries name the state itself, there are no node records.)
// Heap arrays are stored with a one-element bias so that the two children (2i+1, 2i+2) of any node form one naturally
// aligned pair -> a single ds_read_b64 / global_load_dwordx4.
struct TierHbm {
  static constexpr int AS = 1;   // address space of the heaps (and bitmap rows)
  static constexpr int NAS = 1;  // ... of the node records
  static constexpr bool kWideNodes = true;   // four words per node (the position of its open entry in word 3)
  static constexpr bool kPosPair = false;    // TierFocalPos: two words per record, the position in word 1
  static constexpr bool kEntryHasX = false;
  static constexpr bool kEntryXy = false;    // A* tiers: the entry also carries the node's x | y << 8 (TierHybXy)
  static constexpr bool kHybrid = false;
  typedef uint64_t E;
  typedef u64x2 Pair;
  static constexpr uint32_t kFhCap = kFhMax;
  DEVI static E pack(uint32_t fh, uint32_t f, uint32_t g, uint32_t id) {
    const uint32_t key = ((kFhMax - fh) << (kGBits + kFBits)) | ((kFMax - f) << kGBits) | g;
    return ((uint64_t)key << 32) | id;
  }
  DEVI static uint32_t keyFocal(E e) { return (uint32_t)(e >> 32); }
  DEVI static uint32_t keyOpen(E e) { return (uint32_t)(e >> 32) & kOpenKeyMask; }
  DEVI static uint32_t id(E e) { return (uint32_t)e; }
  DEVI static uint32_t f(E e) { return kFMax - ((keyFocal(e) >> kGBits) & kFMax); }
  DEVI static uint32_t g(E e) { return keyFocal(e) & kGMask; }
  DEVI static uint32_t fh(E e) { return kFhMax - (keyFocal(e) >> (kGBits + kFBits)); }
  // walk-queue entry of the ordered walk: the open key of an open-array element and its index
  DEVI static E aux(uint32_t openKey, uint32_t idx) { return ((uint64_t)openKey << 32) | idx; }
  DEVI static uint32_t auxIdx(E e) { return (uint32_t)e; }
  DEVI static E first(E v) { return rfl64(v); }
  DEVI static E fromLane(E v, uint32_t srcLane) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, srcLane);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), srcLane);
    return ((uint64_t)hi << 32) | lo;
  }
  DEVI static E shr1(E v) { return ((uint64_t)waveShr1((uint32_t)(v >> 32)) << 32) | waveShr1((uint32_t)v); }
};

// ---- the arena tier of the CBS / ECBS kernels: heaps whose first nTop entries (their top levels) live in LDS ----------
// After a search has left the compact LDS tier its 13 KB of LDS would sit idle while every heap operation walks arrays in
// HBM, root first.  TierHyb keeps entries [0, nTop) of the open list, the focal list and the walk queue in that LDS and
// the rest in the arena: the roots, the first sift-down block and most of every sift-up chain cost no memory round trip
// at all, and a heap that has at most nTop entries never leaves LDS.  nTop is odd, so an aligned child pair (c, c + 1),
// c odd, lies on one side.  nTop = 0 (no LDS tier configured) degenerates to the plain arena tier.
struct HybRef {
  __attribute__((address_space(3))) uint64_t* top;
  uint64_t* rest;
  uint32_t nTop, i;
  DEVI operator uint64_t() const { return i < nTop ? top[i] : rest[i]; }
  DEVI void operator=(uint64_t e) const {
    if (i < nTop)
      top[i] = e;
    else
      rest[i] = e;
  }
};
struct HybPtr {
  __attribute__((address_space(3))) uint64_t* top;  // element i at top[i] (biased like the arena pointers)
  uint64_t* rest;
  uint32_t nTop;
  DEVI HybRef operator[](uint32_t i) const { return HybRef{top, rest, nTop, i}; }
};
struct TierHyb : TierHbm {
  static constexpr bool kHybrid = true;
};
// ... and, for arenas of at most 65 536 nodes (the conflict-tree drivers' default), the node id takes 16 bits of the
// entry's low word and the node's x | y << 8 the other 16: the expansion then knows its cell from the entry alone and
// requests its bitmap word and the other agents' rows TOGETHER with the node record (which it still needs for the open
// position) instead of after it — one memory round trip less per expansion.
struct TierHybXy : TierHbm {
  static constexpr bool kHybrid = true;
  static constexpr bool kEntryXy = true;
  DEVI static uint32_t id(E e) { return (uint32_t)e & 0xFFFFu; }
  DEVI static uint32_t xyOf(E e) { return ((uint32_t)e >> 16) & 0xFFFFu; }
  DEVI static E withXy(E e, uint32_t xy) { return e | ((uint64_t)(xy & 0xFFFFu) << 16); }
};

// MRP_LL_ASTAR_EPS_TA (runJobTaEps): the FOCAL list of a search whose nodes can be re-keyed while they sit in it.  Same
// entries as TierHbm; `nodes` of its Mem view is a second record per node, {focalH, position of its entry in the focal
// array}, so that POS = true on the focal heap keeps handle -> focal position the way the open heap keeps word 3.
struct TierFocalPos : TierHbm {
  static constexpr bool kPosPair = true;
};

template <class T, bool HYB = T::kHybrid>
struct HeapPtr {
  typedef __attribute__((address_space(T::AS))) typename T::E* type;
};
template <class T>
struct HeapPtr<T, true> {
  typedef HybPtr type;
};

template <class T>
struct Mem {
  typedef typename T::E E;
  typedef typename HeapPtr<T>::type PE;
  typedef __attribute__((address_space(T::AS))) typename T::Pair* PPair;
  typedef __attribute__((address_space(T::AS))) uint32_t* P32;
  typedef __attribute__((address_space(T::AS))) uint16_t* P16;
  typedef __attribute__((address_space(T::NAS))) uint32_t* PN32;
  typedef __attribute__((address_space(T::NAS))) u32x4* PNode4;
  PN32 nodes;     // TierHbm: four words per node; TierLdsSipp: one word per node
  P16 pos;       // TierLdsSipp only: position of the node's entry in the open array
  P16 gOf;       // TierLdsSipp only: arrival time of the node
  PE open;       // biased: element i at open[i] (the pointer already includes the +1 bias)
  PE focal;
  PE aux;        // std::priority_queue of the ordered walk
  P32 bits;      // (time, cell) bitmap: 1 = obstacle | vertex constraint | already discovered
  uint32_t capNodes, capHeap, capRows, rowWords;  // capHeap: entries per heap array (open / focal / walk queue)
};

// The arrays of `m` seen through another tier's types: node records and capacities are copied; the bitmap and the heap
// pointers too where U keeps them in the same kind of memory, and are left null for the caller to set where it does not.
template <class U, class T>
DEVI Mem<U> viewAs(const Mem<T>& m) {
  static_assert(U::NAS == T::NAS, "the node records stay where they are");
  Mem<U> v = {};
  v.nodes = m.nodes;
  if constexpr (U::AS == T::AS) v.bits = m.bits;
  if constexpr (std::is_same<typename Mem<U>::PE, typename Mem<T>::PE>::value) {
    v.open = m.open; v.focal = m.focal; v.aux = m.aux;
  }
  v.capNodes = m.capNodes; v.capHeap = m.capHeap; v.capRows = m.capRows; v.rowWords = m.rowWords;
  return v;
}

template <class T>
DEVI void setPos(Mem<T>& m, uint32_t id, uint32_t idx) {
  if constexpr (T::kPosPair)
    m.nodes[id * 2 + 1] = idx;
  else if constexpr (!T::kWideNodes)
    m.pos[id] = (uint16_t)idx;
  else
    m.nodes[id * 4 + 3] = idx;
}
// x | y << 8 of a node and the position of its entry in the open array (both wave-uniform)
template <class T>
DEVI void nodeXyPos(Mem<T>& m, uint32_t id, uint32_t& xy, uint32_t& pos) {
  static_assert(T::kWideNodes, "arena node records");
  const u32x4 nd = ((typename Mem<T>::PNode4)m.nodes)[id];
  xy = rfl(nd.x) & 0xFFFFu;
  pos = rfl(nd.w);
}
template <class T>
DEVI void nodeXyParent(Mem<T>& m, uint32_t id, uint32_t& xy, uint32_t& parent) {
  static_assert(T::kWideNodes, "arena node records");
  const u32x4 nd = ((typename Mem<T>::PNode4)m.nodes)[id];
  xy = rfl(nd.x) & 0xFFFFu;
  parent = rfl(nd.y);
}

struct Ctx {  // wave-uniform job context
  uint32_t dimx, dimy, wpr, gx, gy, sx, sy;
  int32_t lastGoal;
  float w;
  uint32_t nVc, nEc;
  const uint32_t* vc;       // generic pointers: LDS, arena copy, or (oversized lists only) host memory
  const uint32_t* ec;
  const uint32_t* obst;     // global obstacle bitmap
  const uint16_t* paths;    // generic: LDS copy, arena copy, or host memory
  __attribute__((address_space(3))) const uint16_t* pathsLds;  // the same table when it is the LDS copy (ds_read), else null
  uint32_t nAgentsPad, tPad;
  int64_t maxExp;
  volatile uint32_t* debug;
};

struct SState {  // wave-uniform search state (kept in SGPRs by construction)
  uint32_t nNodes, nOpen, nFocal, rowsReady;
  int32_t bestF;
  int64_t expansions;
};

constexpr int32_t ST_CAP_FOCAL = 7;

template <class T>
DEVI typename T::E ldU(typename Mem<T>::PE p, uint32_t i) { return T::first(p[i]); }

// the aligned pair (i, i + 1), i odd: one load
template <class T>
DEVI typename T::Pair hLoadPair(typename Mem<T>::PE p, uint32_t i) {
  if constexpr (T::kHybrid) {
    if (i < p.nTop) return *(__attribute__((address_space(3))) u64x2*)(p.top + i);
    return *(u64x2*)(p.rest + i);
  } else {
    return *(typename Mem<T>::PPair)(p + i);
  }
}

template <class T>
DEVI void ldPair(typename Mem<T>::PE p, uint32_t i, typename T::E& a, typename T::E& b) {  // i odd -> aligned pair
  const typename T::Pair v = hLoadPair<T>(p, i);
  a = T::first(v.x);
  b = T::first(v.y);
}

// ---- heap primitives ------------------------------------------------------------------------------------------
// The heaps are replayed EXACTLY (same array layout after every operation as boost::heap::d_ary_heap / libstdc++'s
// std::push_heap / std::pop_heap would have), but not one element at a time: the data-independent part of every
// operation is done by all lanes at once so that an operation costs O(1) memory round trips instead of O(log n):
//   * sift-up      : lane k loads the k-th ancestor; one ballot finds where the sequential loop would have stopped;
//                    the ancestors below that point move down one level in a single parallel store.
//   * sift-down    : which child is "the larger one" does not depend on the element being sifted, so 63 lanes load
//                    the child pairs of a whole 6-level subtree in one instruction and every lane then decides from
//                    two ballots whether its node is on the path (followPath: no further memory latency, no scalar
//                    walk); repeated per 6 levels.
//   * erase        : the unconditional bubble-to-root is a one-level shift of the ancestor chain (parallel).
// KEY selects the comparator: 0 = open (f asc, g desc), 1 = focal (focalH, f asc, g desc), 2 = walk queue (an open key
// in the entry's key field).  POS=true maintains handle -> position for the node (open list only).
template <class T, int KEY>
DEVI uint32_t keyOf(typename T::E e) { return KEY == 0 ? T::keyOpen(e) : T::keyFocal(e); }
template <class T, int KEY>
DEVI bool kLess(typename T::E a, typename T::E b) {  // the reference's "operator<": a is WORSE than b
  return keyOf<T, KEY>(a) < keyOf<T, KEY>(b);
}

template <class T, bool POS>
DEVI void heapStore(Mem<T>& m, typename Mem<T>::PE heap, uint32_t idx, typename T::E e) {
  heap[idx] = e;
  if (POS) setPos<T>(m, T::id(e), idx);
}

// boost siftup / libstdc++ __push_heap from position idx: while less(parent, e) the parent moves down.
template <class T, int KEY, bool POS>
DEVI void siftUp(Mem<T>& m, typename Mem<T>::PE heap, uint32_t idx, typename T::E e) {
  typedef typename T::E E;
  const uint32_t lane = threadIdx.x;
  const uint32_t depth = 31u - (uint32_t)__builtin_clz(idx + 1);  // number of ancestors of idx
  uint32_t stop = 0;
  if (depth != 0) {
    const bool act = lane < depth;
    const uint32_t anc = act ? ((idx + 1) >> (lane + 1)) - 1 : 0;     // lane k: k-th ancestor
    const E ae = heap[anc];
    const uint64_t worse = ballot64(act && kLess<T, KEY>(ae, e));
    stop = (uint32_t)__builtin_ctzll(~worse);                          // first ancestor that is not worse than e
    if (lane < stop) {                                                 // ancestors 0..stop-1 move down one level
      const uint32_t dest = ((idx + 1) >> lane) - 1;
      heap[dest] = ae;
      if (POS) setPos<T>(m, T::id(ae), dest);
    }
  }
  heapStore<T, POS>(m, heap, ((idx + 1) >> stop) - 1, e);
}

// Which nodes of a 6-level block lie on the sift-down path, decided by all lanes at once instead of a scalar walk
// over the masks: node l (lane l < 63; 1-based number n = l + 1) is reached iff every ancestor lets the hole pass
// (`go`) and turned towards l (`right` bit == the matching digit of n).  The ancestors of a node of a 63-node tree are
// among its first 31 nodes, so both tests are 32-bit masks that depend on the lane only.
//   anc   : bit a set  <=>  node a is an ancestor of this lane's node
//   needR : bit a set  <=>  ... and the path to this lane's node leaves a through its RIGHT child
struct PathLanes {
  uint32_t anc, needR;
};
DEVI PathLanes pathLanes() {
  const uint32_t n = threadIdx.x + 1;
  PathLanes pl;
  pl.anc = 0;
  pl.needR = 0;
#pragma unroll
  for (uint32_t k = 1; k <= 5; ++k) {
    const uint32_t a = n >> k;  // 1-based number of the k-th ancestor (0: none)
    if (a != 0 && n < 64) {
      pl.anc |= 1u << (a - 1);
      pl.needR |= ((n >> (k - 1)) & 1u) << (a - 1);
    }
  }
  return pl;
}
// Follows the path of one block: `go` / `right` are this lane's answers for its node.  Returns the lanes on the path
// (each pulls its chosen child up), the number of levels descended and the new hole relative to the block's root.
DEVI bool followPath(const PathLanes& pl, bool go, bool right, uint32_t& steps, uint32_t& rel) {
  const uint64_t goMask = ballot64(go);
  const uint64_t rightMask = ballot64(right);
  const uint32_t goLo = (uint32_t)goMask, rLo = (uint32_t)rightMask;
  const bool reached = ((goLo & pl.anc) == pl.anc) && (((rLo ^ pl.needR) & pl.anc) == 0u);
  const bool onPath = reached && go;
  const uint64_t pathMask = ballot64(onPath);
  steps = (uint32_t)__popcll(pathMask);
  rel = 0;
  if (pathMask) {
    const uint32_t d = 63u - (uint32_t)__builtin_clzll(pathMask);  // deepest node on the path (levels are index-ordered)
    rel = 2 * d + 1 + (uint32_t)((rightMask >> d) & 1ull);
  }
  return onPath;
}

// Moves the hole at `idx` down a heap of n elements.
//   STL=false (boost siftdown): prefer the FIRST maximal child; stop in front of a child that is less than x; x is
//             stored at the final hole.
//   STL=true  (libstdc++ __adjust_heap): prefer the right child unless it is less than the left one; always descend
//             to a leaf; the final hole index is returned (the caller then sifts its value up from there).
// Per 6 levels: one pair load per lane (63 lanes = the whole subtree below the hole), two ballots, a scalar walk
// over the two bit masks, and ONE predicated store in which every node on the path pulls its chosen child up.
template <class T, int KEY, bool POS, bool STL>
DEVI uint32_t descend(Mem<T>& m, typename Mem<T>::PE heap, uint32_t n, uint32_t idx, typename T::E x) {
  typedef typename T::E E;
  const uint32_t lane = threadIdx.x;
  const uint32_t lv = 31u - (uint32_t)__builtin_clz(lane + 1);  // level of this lane inside a 6-level subtree
  const uint32_t off = (lane + 1) - (1u << lv);                 // position inside that level
  const uint32_t xk = keyOf<T, KEY>(x);
  const PathLanes pl = pathLanes();
  for (;;) {
    const uint32_t node = ((idx + 1) << lv) - 1 + off;          // lane l < 63 owns this node of the subtree
    const uint32_t c = 2 * node + 1;
    const bool has = (lane < 63) && (c < n);
    typename T::Pair pr;
    pr.x = 0;
    pr.y = 0;
    if (has) pr = hLoadPair<T>(heap, c);                        // children (c, c+1): one aligned load
    const uint32_t kl = keyOf<T, KEY>(pr.x);
    const uint32_t kr = keyOf<T, KEY>(pr.y);
    const bool hasR = has && (c + 1 < n);
    const bool right = hasR && (STL ? !(kr < kl) : (kl < kr));
    const E pe = right ? pr.y : pr.x;
    const uint32_t pk = right ? kr : kl;
    const bool go = has && (STL || !(pk < xk));                 // the hole moves below this node
    uint32_t rel, steps;
    if (followPath(pl, go, right, steps, rel)) {                // every node on the path pulls its chosen child up
      heap[node] = pe;
      if (POS) setPos<T>(m, T::id(pe), node);
    }
    idx = ((idx + 1) << steps) - 1 + (rel + 1 - (1u << steps)); // absolute index of the new hole
    if (steps < 6) break;
  }
  if (!STL) heapStore<T, POS>(m, heap, idx, x);
  return idx;
}

// boost pop: swap(front, back), drop back, siftdown(0)
template <class T, int KEY, bool POS>
DEVI void heapPop(Mem<T>& m, typename Mem<T>::PE heap, uint32_t& n) {
  n -= 1;
  if (n == 0) return;
  const typename T::E last = ldU<T>(heap, n);
  descend<T, KEY, POS, false>(m, heap, n, 0, last);
}

// ---- batched operations of one expansion ------------------------------------------------------------------------
// An expansion pops one element and pushes up to five.  Done one heap operation at a time that is a chain of ~25
// dependent memory round trips; the results of the operations, however, depend on each other only through a handful
// of heap entries, so the loads of ALL of them are issued first and the sequential semantics are then resolved in
// registers:
//   * pushes: the sift-up chain of the k-th new element is held LEVEL-MAJOR — lane L owns the chain's node at tree
//     level L (root = level 0), for every k.  Two chains that pass through the same heap position do so at the same
//     level, i.e. in the same lane, so "what did an earlier push of this expansion leave at this position" is a
//     per-lane select; the one-level move of the ancestors that a sift-up performs is a one-lane shift of the wave
//     (DPP wave_shr:1).  Five pushes into two heaps cost one round trip.
//   * pops: the loads of the focal and the open sift-down (which child is the larger one does not depend on the
//     element being sifted) are issued together, and the moved "last" elements are fetched with them.
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

template <class T>
struct PushChains {          // sift-up chains of the (up to five) pushes of one expansion into one heap
  typedef typename T::E E;
  uint32_t pos[5];           // lane L: heap position of the chain's node at level L (kNoPos: none)
  E val[5];                  // lane L: the entry there before any of these pushes
  // `mask` bit k: successor k is pushed; pushed elements take positions n0, n0+1, ... in ascending k
  DEVI void load(typename Mem<T>::PE heap, uint32_t n0, uint32_t mask) {
    const uint32_t lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      pos[k] = kNoPos;
      val[k] = 0;
      if ((mask >> k) & 1u) {
        const uint32_t p = n0 + (uint32_t)__builtin_popcount(mask & ((1u << k) - 1u));
        const uint32_t d = 31u - (uint32_t)__builtin_clz(p + 1);  // level of p == number of ancestors
        if (lane <= d) pos[k] = ((p + 1) >> (d - lane)) - 1;
        if (lane < d) val[k] = heap[pos[k]];
      }
    }
  }
  // boost siftup / libstdc++ __push_heap of e[k] at its position, for k ascending — the same stores a one-at-a-time
  // replay ends with (positions written twice are written in push order).
  template <int KEY, bool POS>
  DEVI void resolve(Mem<T>& m, typename Mem<T>::PE heap, uint32_t n0, uint32_t mask, const E (&e)[5]) {
    const uint32_t lane = threadIdx.x;
    E nv[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      nv[k] = 0;
      if ((mask >> k) & 1u) {
        const uint32_t p = n0 + (uint32_t)__builtin_popcount(mask & ((1u << k) - 1u));
        const uint32_t d = 31u - (uint32_t)__builtin_clz(p + 1);
        E v = val[k];
#pragma unroll
        for (int j = 0; j < k; ++j)  // what earlier pushes of this expansion left on this chain
          if (((mask >> j) & 1u) && pos[j] == pos[k] && pos[k] != kNoPos) v = nv[j];
        const uint64_t worse = ballot64(lane < d && kLess<T, KEY>(v, e[k]));
        const uint64_t notWorse = ~worse & ((1ull << d) - 1ull);
        const int32_t sLvl = notWorse ? 63 - (int32_t)__builtin_clzll(notWorse) : -1;  // deepest ancestor that stays
        const E sh = T::shr1(v);
        const E nk = (int32_t)lane <= sLvl ? v : ((int32_t)lane == sLvl + 1 ? e[k] : sh);
        if ((int32_t)lane > sLvl && lane <= d) {
          heap[pos[k]] = nk;
          if (POS) setPos<T>(m, T::id(nk), pos[k]);
        }
        nv[k] = nk;
      }
    }
  }
};

// One 6-level block of a sift-down whose child pairs have been loaded (see descend): follows the path, pulls the
// chosen children up, returns the new hole; `more` = the block was left through its bottom.
template <class T, int KEY, bool POS>
DEVI uint32_t descendBlock(Mem<T>& m, typename Mem<T>::PE heap, const PathLanes& pl, uint32_t idx, uint32_t xk,
                           typename T::Pair pr, uint32_t node, bool has, bool hasR, bool& more) {
  typedef typename T::E E;
  const uint32_t kl = keyOf<T, KEY>(pr.x);
  const uint32_t kr = keyOf<T, KEY>(pr.y);
  const bool right = hasR && (kl < kr);
  const E pe = right ? pr.y : pr.x;
  const uint32_t pk = right ? kr : kl;
  const bool go = has && !(pk < xk);
  uint32_t rel, steps;
  if (followPath(pl, go, right, steps, rel)) {
    heap[node] = pe;
    if (POS) setPos<T>(m, T::id(pe), node);
  }
  more = steps == 6;
  return ((idx + 1) << steps) - 1 + (rel + 1 - (1u << steps));
}

// a_star_epsilon.hpp:191-192 of one expansion: focalSet.pop() and openSet.erase(handle of the same node), with the
// memory traffic of the two heaps overlapped.  curPos = position of the popped node in the open array.
template <class T>
DEVI void popFocalEraseOpen(Mem<T>& m, uint32_t& nFocal, uint32_t& nOpen, uint32_t curPos) {
  typedef typename T::E E;
  typedef typename T::Pair Pair;
  const uint32_t lane = threadIdx.x;
  const uint32_t lv = 31u - (uint32_t)__builtin_clz(lane + 1);
  const uint32_t off = (lane + 1) - (1u << lv);
  const PathLanes pl = pathLanes();
  // ---- loads that depend on nothing but the sizes
  nFocal -= 1;
  const uint32_t nOld = nOpen;
  nOpen -= 1;
  E lastFv = 0, lastOv = 0;
  if (nFocal > 0) lastFv = m.focal[nFocal];
  if (nOpen > 0) lastOv = m.open[nOld - 1];
  const uint32_t depth = 31u - (uint32_t)__builtin_clz(curPos + 1);
  const bool act = lane < depth;
  const uint32_t anc = act ? ((curPos + 1) >> (lane + 1)) - 1 : 0;
  E ae = 0;
  if (depth != 0) ae = m.open[anc];
  // first block of the focal sift-down: does not depend on the element being sifted
  uint32_t idxF = 0, idxO = 0;
  bool moreF = nFocal > 0, moreO = nOpen > 0;
  Pair prF;
  prF.x = 0; prF.y = 0;
  const uint32_t nodeF0 = (1u << lv) - 1 + off;
  const bool hasF0 = moreF && lane < 63 && (2 * nodeF0 + 1 < nFocal);
  if (hasF0) prF = hLoadPair<T>(m.focal, 2 * nodeF0 + 1);
  // ---- open: every ancestor of curPos moves down one level (boost erase = bubble to the root, then pop)
  if (act) {
    const uint32_t dest = ((curPos + 1) >> lane) - 1;
    m.open[dest] = ae;
    setPos<T>(m, T::id(ae), dest);
  }
  // the element that pop() moves to the root: the last one — which the shift above has just overwritten if the erased
  // node WAS the last one (then it is the erased node's parent)
  E lastO = T::first(lastOv);
  if (curPos == nOld - 1 && depth != 0) lastO = T::fromLane(ae, 0);
  const E lastF = T::first(lastFv);
  const uint32_t xkF = T::keyFocal(lastF), xkO = T::keyOpen(lastO);
  // ---- sift-downs, block by block, both heaps per round trip
  bool firstF = true;
  for (;;) {
    Pair prO;
    prO.x = 0; prO.y = 0;
    const uint32_t nodeO = ((idxO + 1) << lv) - 1 + off;
    const bool hasO = moreO && lane < 63 && (2 * nodeO + 1 < nOpen);
    if (hasO) prO = hLoadPair<T>(m.open, 2 * nodeO + 1);
    uint32_t nodeF = nodeF0;
    bool hasF = hasF0;
    if (!firstF) {
      nodeF = ((idxF + 1) << lv) - 1 + off;
      hasF = moreF && lane < 63 && (2 * nodeF + 1 < nFocal);
      prF.x = 0; prF.y = 0;
      if (hasF) prF = hLoadPair<T>(m.focal, 2 * nodeF + 1);
    }
    firstF = false;
    if (moreF)
      idxF = descendBlock<T, 1, false>(m, m.focal, pl, idxF, xkF, prF, nodeF, hasF, hasF && (2 * nodeF + 2 < nFocal), moreF);
    if (moreO)
      idxO = descendBlock<T, 0, true>(m, m.open, pl, idxO, xkO, prO, nodeO, hasO, hasO && (2 * nodeO + 2 < nOpen), moreO);
    if (!moreF && !moreO) break;
  }
  if (nFocal > 0) m.focal[idxF] = lastF;
  if (nOpen > 0) heapStore<T, true>(m, m.open, idxO, lastO);
}

// ---- ordered walk (open.ordered_begin(), a_star_epsilon.hpp:141-152) ----------------------------------------
// libstdc++ std::priority_queue<…> restated: push = __push_heap, pop = __pop_heap/__adjust_heap (bits/stl_heap.h).
template <class T>
DEVI typename T::E auxPop(Mem<T>& m, uint32_t& npq) {
  typedef typename T::E E;
  const E result = ldU<T>(m.aux, 0);
  npq -= 1;
  if (npq > 0) {
    const E value = ldU<T>(m.aux, npq);  // *(last - 1)
    const uint32_t hole = descend<T, 2, false, true>(m, m.aux, npq, 0, value);
    siftUp<T, 2, false>(m, m.aux, hole, value);
  }
  return result;  // open key and index into the open array
}

template <class T>
DEVI void orderedWalk(Mem<T>& m, SState& s, const Ctx& c, int32_t oldBest, DevResult& res) {
  typedef typename T::E E;
  // int * float products in binary32, no contraction (a_star_epsilon.hpp:145,149)
  const float lo = __fmul_rn((float)oldBest, c.w);
  const float hi = __fmul_rn((float)s.bestF, c.w);
  // The queue entry of a visited element carries its open key, so f is known without touching the open array again;
  // the two children are pushed with one round trip (PushChains).  In a long search the walks are most of the time
  // (every bestF increase visits every open node with f <= hi), so a round trip per visited node matters.
  uint32_t npq = 0;
  E curA = T::aux(T::keyOpen(ldU<T>(m.open, 0)), 0);  // index 0
  for (;;) {
    const uint32_t cur = T::auxIdx(curA);
    const uint32_t first = 2 * cur + 1;
    if (first < s.nOpen) {
      E e1, e2;
      ldPair<T>(m.open, first, e1, e2);
      E ee[5];
      ee[0] = T::aux(T::keyOpen(e1), first);
      ee[1] = T::aux(T::keyOpen(e2), first + 1);
      ee[2] = ee[3] = ee[4] = 0;
      const uint32_t pm = first + 1 < s.nOpen ? 3u : 1u;
      PushChains<T> pc;
      pc.load(m.aux, npq, pm);
      pc.template resolve<2, false>(m, m.aux, npq, pm, ee);  // == __push_heap of the children in index order
      npq += pm == 3u ? 2u : 1u;
    }
    PROF_INC(res, 7, 1);

    const float fv = (float)(int32_t)T::f(curA);
    if (fv > lo && fv <= hi) {
      const E e = ldU<T>(m.open, cur);
      siftUp<T, 1, false>(m, m.focal, s.nFocal, e);
      s.nFocal += 1;
    }
    if (fv > hi) break;
    if (npq == 0) break;
    curA = auxPop<T>(m, npq);
  }
}

}  // namespace mrp

#endif  // MRP_LL_ARENA_HEAP_H
