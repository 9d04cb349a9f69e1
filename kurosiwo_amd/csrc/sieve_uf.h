// Lock-free union-find over an int32 parent array, and the vote arg-max of the sieve (sieve.hip).  Host and device: the helpers are
// templates over a small "memory" policy (load, fetch-min), so a host program can run the same tile and border merges sequentially
// on a plain array, while the kernels run them on LDS (workgroup-scope atomics) and on global memory (agent-scope atomics).
//
// Invariant: parent[i] <= i at every moment, and a cell is only ever LOWERED (fetch-min).  i is a root while parent[i] == i.
//   uf_find   follows parent links while they strictly decrease; every step lowers x by at least 1, so at most x steps.  A cell that
//             does not point strictly below itself ends the walk (a root; a value above the index cannot arise and would end it too).
//   uf_union  takes the two roots a > b and lowers parent[a] to b with one fetch-min.  When the fetch-min returns a itself, a was a
//             root and now hangs below b: done.  Otherwise another union lowered parent[a] first and the fetch-min returned that
//             label `old` < a; the link a -> old may just have been replaced by a -> b, so the pending equivalence is (old, b) and the
//             loop continues with it.  It retries ONLY in that case, and then max(a, b) has strictly decreased (old < a, and the finds
//             only go down), so the loop runs at most a + b times whatever other threads do.  No locks, no waiting on another thread.
// The root of a finished component is the smallest index in it, since a union always hangs the larger root below the smaller one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KSMI_HD __host__ __device__ __forceinline__
#else
#define KSMI_HD inline
#endif

// plain memory: the sequential host build
struct uf_plain_mem {
  int32_t* p;
  KSMI_HD int32_t load(int32_t i) const { return p[i]; }
  KSMI_HD int32_t fetch_min(int32_t i, int32_t v) const {
    const int32_t old = p[i];
    if (v < old) p[i] = v;
    return old;
  }
};

template <class Mem>
KSMI_HD int32_t uf_find(const Mem& m, int32_t x) {
  for (;;) {
    const int32_t p = m.load(x);
    if (p >= x) return x;
    x = p;
  }
}

template <class Mem>
KSMI_HD void uf_union(const Mem& m, int32_t a, int32_t b) {
  for (;;) {
    a = uf_find(m, a);
    b = uf_find(m, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = m.fetch_min(a, b);
    if (old >= a) return;        // a was a root and now points at b
    a = old;                     // lowered by someone else in the meantime: carry (old, b) on
  }
}

// the class with the most votes, the lowest index on a tie; -1 when nobody voted.  v(k) = votes of class k
template <class Votes>
KSMI_HD int sieve_vote_argmax(const Votes& v, int K) {
  int best = -1;
  int32_t most = 0;
  for (int k = 0; k < K; ++k) {
    const int32_t n = v(k);
    if (n > most) {
      most = n;
      best = k;
    }
  }
  return best;
}

// a class value that the sieve neither changes nor lets vote: the invalid class, and any value the vote table has no row for
KSMI_HD bool sieve_is_invalid(int c, int invalid_class, int K) { return c == invalid_class || c >= K; }
