// rse_read_plan.hpp -- the arithmetic of one rse_read_flat or rse_read_shards
// call: which codecs it takes, when an entry of the read list is in order, how a run's entries
// are cut into output groups, whether the kernel may take its 16-byte path, how
// many workgroups are launched, and the plan of one run: from a stripe's flag
// row and the shards wanted of it, the valid set, every entry's class and, for
// a rebuilt entry, its k coefficients over the valid set.  Run heads, spans
// and lanes are rse_update_plan.hpp's.  Plain C++, __host__ __device__ under
// hipcc: the device passes (rse_read.hip) call the functions the CPU tests
// walk (tests/native/read_plan.cpp, read_shards_plan.cpp).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rse_update_plan.hpp"

namespace rse {

// Which codecs rse_read_flat takes: rse_update_flat's, with at most kReadMaxP
// parity shards -- at most that many data shards are rebuilt, so the [A | I]
// elimination of a run (read_plan_run) fits a workgroup's LDS as bytes.
constexpr uint32_t kReadMaxP = 128, kReadMaxShards = 256;
inline bool read_in_scope(int field, size_t k, size_t p) {
  return update_in_scope(field, k, p) && p <= kReadMaxP;
}

// The list: entry u is the words {stripe, shard} at reads[2u], reads[2u + 1],
// any of the stripe's k + p shards.  In order: rse_update_flat's rule with
// k + p in the place of k.
RSE_UPD_HD bool read_in_order(const uint32_t* reads, uint64_t u, uint32_t n_stripes,
                              uint32_t total) {
  return update_in_order(reads, u, n_stripes, total);
}

// A run's entries in output groups of kReadRows: a work item keeps one group's
// rows in registers.  Every group but a run's last is full.
constexpr uint32_t kReadRows = 16;
RSE_UPD_HD uint32_t read_groups(uint32_t entries) { return (entries + kReadRows - 1) / kReadRows; }
RSE_UPD_HD uint32_t read_group_first(uint32_t g) { return g * kReadRows; }
RSE_UPD_HD uint32_t read_group_entries(uint32_t entries, uint32_t g) {
  const uint32_t first = g * kReadRows;
  return entries - first < kReadRows ? entries - first : kReadRows;
}
// The longest run there can be: no entry twice, so a stripe's shards at most.
RSE_UPD_HD uint32_t read_max_run(uint64_t n_reads, uint32_t total) {
  return n_reads < total ? (uint32_t)n_reads : total;
}

// The 16-byte path: every shard of `stripes` and every row of `out` starts on
// a 16-byte boundary and ends on one.
inline bool read_vec(const void* stripes, const void* out, uint64_t shard_bytes) {
  return update_vec(stripes, out, shard_bytes);
}

// rse_read_shards' 16-byte path: every shard pointer that is there and `out`
// start on a 16-byte boundary, and a block's bytes and a shard's bytes are
// multiples of 16 -- so every block and every row start on a boundary and the
// shorter last block ends on one.  A NULL pointer (a shard without a buffer)
// decides nothing: no address is formed from it.
inline bool read_shards_vec(const void* const* ptrs, size_t n, const void* out,
                            uint64_t block_bytes, uint64_t len_bytes) {
  bool al = reinterpret_cast<uintptr_t>(out) % 16u == 0 && block_bytes % 16u == 0 &&
            len_bytes % 16u == 0;
  for (size_t i = 0; i < n; ++i)
    al = al && (ptrs[i] == nullptr || reinterpret_cast<uintptr_t>(ptrs[i]) % 16u == 0);
  return al;
}

// Workgroups of the read kernel, which steps over (run, group, span) items in
// grid strides: RSE_OPT_GRID_X > 0 sets the count outright, else what the
// device holds at once, and no more than the items there can be -- a group has
// at least one entry, so at most one (run, group) per entry.
inline uint32_t read_grid(uint32_t cus, int64_t grid_opt, uint64_t n_reads, uint64_t shard_bytes) {
  return update_grid(cus, grid_opt, n_reads, shard_bytes);
}

// ---- the plan of one run

constexpr uint8_t kReadCopied = 0, kReadRebuilt = 1, kReadLost = 2;  // RSE_READ_*

RSE_UPD_HD uint32_t read_gf_mul(const uint8_t* lg, const uint8_t* ex, uint32_t a, uint32_t b) {
  return (a && b) ? ex[(uint32_t)lg[a] + lg[b]] : 0u;
}

// A run's work area: plain arrays on the host, LDS on the device.
struct ReadRunWork {
  uint8_t* fl;     // kReadMaxShards: the flag row, 0 / 1
  uint8_t* where;  // kReadMaxShards: a missing data shard's place in S
  uint8_t* valid;  // kReadMaxShards (k used): the first k present shards, ascending
  uint8_t* S;      // kReadMaxP: the missing data shards, ascending
  uint8_t* R;      // kReadMaxP: the valid set's parity rows (shard - k), ascending
  uint8_t* A;      // e x 2e, e <= kReadMaxP: [P[R][S] | I], then [I | its inverse]
  uint8_t* D;      // e x k: every missing data shard over the valid set
  uint32_t* sc;    // 4 words: shards in the valid set, e, pivot, recoverable
};
constexpr size_t kReadWorkA = (size_t)2 * kReadMaxP * kReadMaxP;  // bytes of A
constexpr size_t kReadWorkD = (size_t)kReadMaxP * kReadMaxP;      // of D: e x k <= p x k <= 128^2

// What a thread team is on the host: one thread, nothing to wait for.
struct ReadNoSync {
  RSE_UPD_HD void operator()() const {}
};

// Which shards have no buffer: erased whatever the flag row says.  Never, for
// the flat layout; for separately allocated shards the pointer table itself is
// asked (rse_read_shards: shards[i] == NULL), so there is nothing beside it
// that could disagree with it.
struct ReadAllBuffers {
  RSE_UPD_HD bool operator()(uint32_t) const { return false; }
};
struct ReadNullShards {
  const uint8_t* const* ptr;  // k + p pointers
  RSE_UPD_HD bool operator()(uint32_t shard) const { return ptr[shard] == nullptr; }
};

// Gauss-Jordan on the e x 2e bytes of w by the team (thread tid of nt; sync()
// is its barrier): the unique inverse, so the pivot choice cannot change the
// result.  False if singular (uniform), which an MDS code never is.
template <class Sync>
RSE_UPD_HD bool read_gauss_jordan(uint8_t* w, uint32_t e, const uint8_t* lg, const uint8_t* ex,
                                  uint32_t* piv_word, uint32_t tid, uint32_t nt, Sync sync) {
  const uint32_t w2 = 2 * e;
  for (uint32_t col = 0; col < e; ++col) {
    if (tid == 0) {
      uint32_t piv = e;
      for (uint32_t r = col; r < e; ++r)
        if (w[r * w2 + col]) {
          piv = r;
          break;
        }
      *piv_word = piv;
    }
    sync();
    const uint32_t piv = *piv_word;
    if (piv == e) return false;
    if (piv != col) {
      for (uint32_t c = tid; c < w2; c += nt) {
        const uint8_t t0 = w[col * w2 + c];
        w[col * w2 + c] = w[piv * w2 + c];
        w[piv * w2 + c] = t0;
      }
      sync();
    }
    const uint32_t inv = ex[255u - lg[w[col * w2 + col]]];
    sync();  // every thread has read the pivot before the row is scaled
    for (uint32_t c = tid; c < w2; c += nt)
      w[col * w2 + c] = (uint8_t)read_gf_mul(lg, ex, inv, w[col * w2 + c]);
    sync();
    for (uint32_t t = tid; t < e * w2; t += nt) {  // eliminate column `col` elsewhere
      const uint32_t r = t / w2, c = t % w2;
      if (r == col || c == col) continue;
      const uint32_t f = w[r * w2 + col];
      if (f) w[t] ^= (uint8_t)read_gf_mul(lg, ex, f, w[col * w2 + c]);
    }
    sync();
    for (uint32_t r = tid; r < e; r += nt)
      if (r != col) w[r * w2 + col] = 0;
    sync();
  }
  return true;
}

// The plan of one run, by a team of nt threads (the host: tid 0 of 1).
//   lg, ex   the GF(2^8) log table (256) and the doubled exp table (>= 510)
//   P        the codec's p x k parity rows as bytes
//   flags    the stripe's k + p flags, non-zero = present; nullptr: all present
//   no_buffer  no_buffer(shard): the shard is erased whatever its flag says
//            (ReadAllBuffers: none is; the overload below passes that)
//   entries  the run's n entries, {stripe, shard} words: entries[2j + 1] is wanted
//   emit     emit.cls(j, class) once per entry, emit.coef(j, i, c) for every
//            rebuilt entry j and every input i < k
// Afterwards w.valid holds the valid set -- the first k present shards in
// index order, so the k - e present data shards and then R, the first e present
// parity rows -- where w.sc[3] says the stripe is recoverable (k shards present).
// Only a shard whose w.fl is set gets into the valid set or is copied, and a
// shard without a buffer never has it set: the read kernel, which takes every
// shard index from the valid set or from a copied entry, forms no address from it.
// A present entry is copied; an erased one of a recoverable stripe is rebuilt,
// else lost.  Coefficients as recon_plan_kernel (rse_kernels.hip) composes them:
// only the e x e matrix A = P[R][S] over the missing data shards S is inverted;
// missing data shard S_u over the valid set is D[u] -- A^-1[u][t] on parity
// input R_t, sum_t A^-1[u][t] P[R_t][d] on present data shard d; missing parity
// shard r is P[r] over the data, the rebuilt data through D:
// [input i is data d] P[r][d] + sum_u P[r][S_u] D[u][i].  Each is the unique
// linear map from the k valid shards to the shard, so the bytes are the
// reference's reconstruct (core.rs:733-923).
template <class Sync, class Emit, class NoBuffer>
RSE_UPD_HD void read_plan_run(const uint8_t* lg, const uint8_t* ex, const uint8_t* P, uint32_t k,
                              uint32_t p, const uint8_t* flags, const uint32_t* entries,
                              uint32_t n, const ReadRunWork& w, Emit& emit, uint32_t tid,
                              uint32_t nt, Sync sync, NoBuffer no_buffer) {
  const uint32_t T = k + p;
  sync();  // the team is done with the run before
  for (uint32_t row = tid; row < T; row += nt)
    w.fl[row] = ((!flags || flags[row]) && !no_buffer(row)) ? 1 : 0;
  sync();
  if (tid == 0) {
    uint32_t nv = 0, ne = 0, nr = 0;
    for (uint32_t row = 0; row < T; ++row) {
      if (w.fl[row]) {
        if (nv < k) {
          w.valid[nv++] = (uint8_t)row;
          if (row >= k) w.R[nr++] = (uint8_t)(row - k);
        }
      } else if (row < k) {
        // more than p missing: not recoverable, S is not used
        if (ne < p) w.S[ne] = (uint8_t)row;
        w.where[row] = (uint8_t)ne++;
      }
    }
    w.sc[0] = nv;
    w.sc[1] = ne;
    w.sc[3] = nv == k ? 1u : 0u;
  }
  sync();
  const uint32_t e = w.sc[1];
  if (w.sc[3] && e) {
    const uint32_t w2 = 2 * e;
    for (uint32_t t = tid; t < e * w2; t += nt) {
      const uint32_t r = t / w2, c = t % w2;
      w.A[t] = c < e ? P[(size_t)w.R[r] * k + w.S[c]] : (uint8_t)((c - e) == r ? 1 : 0);
    }
    sync();
    const bool ok = read_gauss_jordan(w.A, e, lg, ex, &w.sc[2], tid, nt, sync);
    if (!ok && tid == 0) w.sc[3] = 0;
    sync();
    if (ok)
      for (uint32_t t = tid; t < e * k; t += nt) {
        const uint32_t u = t / k, i = t % k, v = w.valid[i];
        uint32_t c = 0;
        if (v >= k) {
          c = w.A[u * w2 + e + (i - (k - e))];
        } else {
          for (uint32_t q = 0; q < e; ++q)
            c ^= read_gf_mul(lg, ex, w.A[u * w2 + e + q], P[(size_t)w.R[q] * k + v]);
        }
        w.D[t] = (uint8_t)c;
      }
    sync();
  }
  const bool recoverable = w.sc[3] != 0;
  for (uint64_t t = tid; t < (uint64_t)n * k; t += nt) {
    const uint32_t j = (uint32_t)(t / k), i = (uint32_t)(t % k), m = entries[2 * (size_t)j + 1];
    const uint8_t cls = w.fl[m] ? kReadCopied : recoverable ? kReadRebuilt : kReadLost;
    if (i == 0) emit.cls(j, cls);
    if (cls != kReadRebuilt) continue;
    uint32_t c;
    if (m < k) {
      c = w.D[(size_t)w.where[m] * k + i];
    } else {
      const uint32_t v = w.valid[i];
      c = v < k ? P[(size_t)(m - k) * k + v] : 0u;
      for (uint32_t u = 0; u < e; ++u)
        c ^= read_gf_mul(lg, ex, P[(size_t)(m - k) * k + w.S[u]], w.D[(size_t)u * k + i]);
    }
    emit.coef(j, i, (uint8_t)c);
  }
}

// Every shard has a buffer: the flat layout.
template <class Sync, class Emit>
RSE_UPD_HD void read_plan_run(const uint8_t* lg, const uint8_t* ex, const uint8_t* P, uint32_t k,
                              uint32_t p, const uint8_t* flags, const uint32_t* entries,
                              uint32_t n, const ReadRunWork& w, Emit& emit, uint32_t tid,
                              uint32_t nt, Sync sync) {
  read_plan_run(lg, ex, P, k, p, flags, entries, n, w, emit, tid, nt, sync, ReadAllBuffers());
}

}  // namespace rse
