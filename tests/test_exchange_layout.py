"""The layout of the persistent kernel's exchange (bpa_exchange_layout, csrc/sampler.hpp; the kernel computes its addresses with
the same function: smp2::xlayout, csrc/sweep2.hpp).  Host code, no GPU.  An accumulator set is S shards, each a 128-byte line of
16 words (15 sums + the arrival word); a workgroup adds to one shard, the polling wave's 64 lanes read every word of every shard
once a round, S/4 loads a lane, and add up what they read per lane and then over the lanes 16 apart — so word k of a shard must
only ever be read by a lane with lane mod 16 = k."""
import ctypes

import pytest

import bpp_amd

LINE = 16                      # 8-byte words of a 128-byte line
SHARDS = (8, 16, 32, 64)
NWG = (1, 7, 8, 9, 63, 64, 65, 250, 448)


def layout(S, wg, lane, load):
    out = (ctypes.c_uint * 4)()
    ret = bpp_amd.lib().bpa_exchange_layout(S, wg, lane, load, out)
    return ret, dict(set_words=out[0], alloc_words=out[1], shard=out[2], word=out[3])


@pytest.mark.parametrize("S", SHARDS)
def test_shards_are_lines_of_their_own_inside_the_allocation(S):
    ret, L0 = layout(S, 0, 0, 0)
    assert ret == S // 4
    set_words, alloc = L0["set_words"], L0["alloc_words"]
    assert 2 * set_words <= alloc
    for nwg in NWG:
        shard_of = {}
        for b in range(nwg):
            ret, L = layout(S, b, 0, 0)
            assert ret == S // 4 and (L["set_words"], L["alloc_words"]) == (set_words, alloc)
            off = L["shard"]
            assert off % LINE == 0
            idx = off // LINE
            assert idx == b % S and idx < S                        # shard b mod S: workgroups of one shard also share b mod 8
            shard_of[b] = off
        # both sets: the second follows the first; every line a workgroup adds to is 128-byte aligned, inside the allocation, and
        # no line of one set is a line of the other
        lines = [[p * set_words + off for off in sorted(set(shard_of.values()))] for p in (0, 1)]
        for p in (0, 1):
            assert len(set(lines[p])) == min(nwg, S)
            assert all(w % LINE == 0 and 0 <= w and w + LINE <= alloc for w in lines[p])
        assert not set(lines[0]) & set(lines[1])


@pytest.mark.parametrize("S", SHARDS)
def test_the_poll_reads_every_word_of_every_shard_once(S):
    shard_lines = sorted({layout(S, b, 0, 0)[1]["shard"] for b in range(S)})
    assert len(shard_lines) == S
    want = {line + k for line in shard_lines for k in range(LINE)}
    seen = {}
    for lane in range(64):
        for load in range(S // 4):
            ret, L = layout(S, 5, lane, load)                # (which workgroup polls does not matter)
            assert ret == S // 4
            w = L["word"]
            assert w not in seen, (lane, load, seen[w])
            seen[w] = (lane, load)
            assert w % LINE == lane % 16                           # word k on the lanes with lane & 15 == k only
            assert w < L["set_words"]
    assert set(seen) == want
    # a lane's loads are equally spaced (the kernel steps a pointer), and the 16 lanes of one load that share lane >> 4 read one line
    for lane in range(64):
        ws = [layout(S, 0, lane, j)[1]["word"] for j in range(S // 4)]
        assert len({b - a for a, b in zip(ws, ws[1:])}) == 1
    for load in range(S // 4):
        for x in range(4):
            assert len({layout(S, 0, 16 * x + k, load)[1]["word"] // LINE for k in range(16)}) == 1
    assert layout(S, 5, 3, 1)[1]["word"] == layout(S, 77, 3, 1)[1]["word"]


def test_arguments_out_of_range():
    out = (ctypes.c_uint * 4)()
    f = bpp_amd.lib().bpa_exchange_layout
    for S in (0, 4, 12, 48, 128):
        assert f(S, 0, 0, 0, out) == 0
    assert f(8, 0, 64, 0, out) == 0
    assert f(8, 0, 0, 2, out) == 0 and f(64, 0, 0, 15, out) == 16 and f(64, 0, 0, 16, out) == 0
    assert f(8, 0, 0, 0, None) == 0
