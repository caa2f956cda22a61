// Multi-tensor launches: one kernel works on MT_CHUNK-element chunks of many tensors at once (AdamW, gradient accumulation,
// the sum of squares of gradient clipping).  The tensor table travels in the kernel arguments -- the gradients' addresses
// change with every backward, a device-resident table would need an upload per call -- so a call is cut into launches of at
// most NT tensors and NB chunks.  Block b works on chunk (map[b] >> 8) of tensor (map[b] & 255).
// The host part is plain C++17 (tests/test_multi_tensor_cpu.py compiles it without HIP).
#pragma once
#include <stddef.h>

constexpr int MT_CHUNK = 32768;

template <class T, int NT, int NB>
struct MtBatch {
  using item = T;
  static constexpr int tensors = NT, blocks = NB;
  T t[NT];
  unsigned map[NB];
};

// Cuts tensors[0..count) (an item has a `long long n`, its element count) into launches of a Batch = MtBatch<T, NT, NB>, greedily in table order: a launch is
// flushed when its NT tensor slots or its NB chunk slots are full.  A tensor that continues in the next launch restarts
// there at local chunk 0 with its base shifted: advance(item, elements) moves the item's pointers forward and reduces its n.
// launch(batch, nblocks, first_chunk) is called once per launch; first_chunk is the index of its first chunk in the call.
template <class Batch, class Advance, class Launch>
void mt_for_each_launch(const typename Batch::item* tensors, int count, Advance advance, Launch launch) {
  constexpr int NT = Batch::tensors, NB = Batch::blocks;
  static_assert(sizeof(Batch) <= 4000, "the tensor table travels in the kernel arguments");
  static_assert(NT <= 256 && NB <= (1 << 24), "map entry: 8 bits of tensor, 24 bits of chunk");
  Batch b;
  int nt = 0, nb = 0;
  long long first_chunk = 0;
  auto flush = [&]() {
    if (nb) launch(b, nb, first_chunk);
    first_chunk += nb;
    nt = nb = 0;
  };
  for (int i = 0; i < count; ++i) {
    const long long chunks = (tensors[i].n + MT_CHUNK - 1) / MT_CHUNK;
    long long c = 0;
    while (c < chunks) {
      if (nt == NT || nb == NB) flush();
      b.t[nt] = tensors[i];
      advance(b.t[nt], c * MT_CHUNK);
      long long local = 0;
      while (c < chunks && nb < NB) {
        b.map[nb++] = (unsigned)nt | ((unsigned)local << 8);
        ++local;
        ++c;
      }
      ++nt;
    }
  }
  flush();
}

#ifdef __HIPCC__
// Device side, first statement of a kernel whose argument `a` is a MtBatch: declares this block's item `t` (a reference), the
// first element `lo` of its chunk within the item and the chunk's element count `cnt`.  A macro, not a function: a helper
// that is handed the kernel-argument struct by reference is optimised apart from the kernel before it is inlined, and the
// kernels then come out with other (equivalent) instructions than with the decode written in place.
#define MT_DECODE_CHUNK(a, t, lo, cnt)                               \
  const unsigned mt_entry_ = (a).map[blockIdx.x];                    \
  const auto& t = (a).t[mt_entry_ & 255u];                           \
  const size_t lo = (size_t)(mt_entry_ >> 8) * MT_CHUNK;             \
  const size_t mt_left_ = (size_t)t.n - lo;                          \
  const int cnt = mt_left_ < (size_t)MT_CHUNK ? (int)mt_left_ : MT_CHUNK
#endif
