"""The host batcher of csrc/multi_tensor.h (AdamW, gradient accumulation and the sum of squares share it), without a GPU: a
host C++ compiler instantiates it for a toy item at the three (tensors, chunks) limits below, the program prints what every
launch would be handed, and the output is checked against the greedy rule restated here."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CHUNK = 32768
LIMITS = [(36, 400), (36, 768), (3, 5)]                  # AdamW / sum of squares, accumulation, small enough to cross both often

_PROGRAM = r"""
#include <stdio.h>
#include "multi_tensor.h"
struct Item { long long base; long long n; };
template <int NT, int NB>
static void run(const Item* items, int count) {
  mt_for_each_launch<MtBatch<Item, NT, NB>>(
      items, count, [](Item& t, long long k) { t.base += k; t.n -= k; },
      [](const MtBatch<Item, NT, NB>& b, int nb, long long first_chunk) {
        int nt = 0;
        for (int i = 0; i < nb; ++i) nt = (int)(b.map[i] & 255u) + 1 > nt ? (int)(b.map[i] & 255u) + 1 : nt;
        printf("launch %d %lld %d\n", nb, first_chunk, nt);
        for (int i = 0; i < nt; ++i) printf("item %lld %lld\n", b.t[i].base, b.t[i].n);
        for (int i = 0; i < nb; ++i) printf("block %u %u\n", b.map[i] & 255u, b.map[i] >> 8);
      });
  printf("end\n");
}
int main(void) {
  static_assert(MT_CHUNK == 32768, "the chunk the Python side assumes");
  int nt, nb, count;
  static Item items[64];
  while (scanf("%d %d %d", &nt, &nb, &count) == 3) {
    if (count > 64) return 2;
    for (int i = 0; i < count; ++i)
      if (scanf("%lld %lld", &items[i].base, &items[i].n) != 2) return 2;
    if (nt == 36 && nb == 400) run<36, 400>(items, count);
    else if (nt == 36 && nb == 768) run<36, 768>(items, count);
    else if (nt == 3 && nb == 5) run<3, 5>(items, count);
    else return 2;
  }
  return 0;
}
"""


def cases(NB):
    return {
        "empty list": [],
        "one element": [1],
        "exactly NB chunks, then NB + 1": [NB * CHUNK, (NB + 1) * CHUNK],
        "37 one-element tensors": [1] * 37,
        "one tensor over three launches, then small ones": [2 * NB * CHUNK + 3 * CHUNK + 7, 5, CHUNK, 3 * CHUNK + 1, 2],
        "chunk - 1, chunk, chunk + 1": [CHUNK - 1, CHUNK, CHUNK + 1],
    }


def greedy(ns, NT, NB):
    """The rule: tensors in order, a tensor's chunks in order; a launch is closed when it holds NT tensors or NB chunks.
    -> per launch [(tensor, its first chunk in this launch, chunks)]."""
    launches, cur, nb = [], [], 0
    for i, n in enumerate(ns):
        c, chunks = 0, -(-n // CHUNK)
        while c < chunks:
            if len(cur) == NT or nb == NB:
                launches, cur, nb = launches + [cur], [], 0
            take = min(chunks - c, NB - nb)
            cur, nb, c = cur + [(i, c, take)], nb + take, c + take
    return launches + [cur] if cur else launches


@pytest.fixture(scope="module")
def batcher(tmp_path_factory):
    """-> run(NT, NB, ns) = the launches the batcher makes for tensors of ns elements: [(first_chunk, items, blocks)]."""
    d = tmp_path_factory.mktemp("multi_tensor")
    (d / "batch.cpp").write_text(_PROGRAM)
    cxx = shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (c++, or the clang++ that hipcc drives)"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "msclip_amd", "csrc"), str(d / "batch.cpp"),
                    "-o", str(d / "batch")], check=True)                      # (no HIP header, no device pass)

    def run(NT, NB, lists):
        text = "".join(f"{NT} {NB} {len(ns)} " + " ".join(f"{i << 40} {n}" for i, n in enumerate(ns)) + "\n" for ns in lists)
        out = subprocess.run([str(d / "batch")], input=text, check=True, capture_output=True, text=True).stdout
        results = []
        for part in out.split("end\n")[:-1]:
            launches = []
            for line in part.splitlines():
                kind, *v = line.split()
                v = [int(x) for x in v]
                if kind == "launch":
                    launches.append({"nb": v[0], "first": v[1], "nt": v[2], "items": [], "blocks": []})
                else:
                    launches[-1][kind + "s"].append(tuple(v))
            results.append(launches)
        assert len(results) == len(lists)
        return results
    return run


@pytest.mark.parametrize("NT,NB", LIMITS)
def test_batcher_partition_is_the_greedy_rule(batcher, NT, NB):
    named = cases(NB)
    for (what, ns), launches in zip(named.items(), batcher(NT, NB, list(named.values()))):
        rule = greedy(ns, NT, NB)
        assert len(launches) == len(rule), what
        covered, chunk_index = [], 0
        for launch, expect in zip(launches, rule):
            assert launch["first"] == chunk_index, what                       # the global chunk index runs on across launches
            assert 1 <= launch["nb"] == len(launch["blocks"]) <= NB and 1 <= launch["nt"] == len(launch["items"]) <= NT, what
            chunk_index += launch["nb"]
            # a continuing tensor restarts at local chunk 0 with a shifted base
            assert launch["items"] == [((i << 40) + c * CHUNK, ns[i] - c * CHUNK) for i, c, _ in expect], what
            assert launch["blocks"] == [(j, k) for j, (_, _, take) in enumerate(expect) for k in range(take)], what
            for j, local in launch["blocks"]:
                base, n = launch["items"][j]
                assert 0 < n - local * CHUNK
                covered.append((base + local * CHUNK, min(CHUNK, n - local * CHUNK)))
        # every element of every tensor exactly once, in order
        assert covered == [((i << 40) + c * CHUNK, min(CHUNK, n - c * CHUNK)) for i, n in enumerate(ns) for c in range(-(-n // CHUNK))], what
        assert chunk_index == sum(-(-n // CHUNK) for n in ns), what
    assert batcher(NT, NB, [[]]) == [[]]                                       # nothing to do: no launch


def test_the_cases_cross_both_limits():
    """The inputs above do what they are for, at the limits the library uses: launches closed by the tensor limit, launches
    closed by the chunk limit, and a tensor in three launches."""
    for NT, NB in LIMITS:
        named = cases(NB)
        assert len(greedy(named["37 one-element tensors"], NT, NB)) == -(-37 // NT)
        assert [len(launch) for launch in greedy(named["exactly NB chunks, then NB + 1"], NT, NB)] == [1, 1, 1]
        spans = greedy(named["one tensor over three launches, then small ones"], NT, NB)
        assert [launch[0][0] for launch in spans[:3]] == [0, 0, 0] and sum(t for launch in spans for _, _, t in launch) == 2 * NB + 11
