"""tests/stream_order.py's checker against hand-written traces (no GPU, no torch.cuda), and the write table against the public
functions of msclip_amd.hip.  Streams are small integers (0 = main, 1 = lane, 2 = a third one), addresses are made up."""
import stream_order as so
from msclip_amd import hip

MAIN, LANE, THIRD = 0, 1, 2
W = (0x1000, 0x2000)                                      # a persistent buffer (weights / workspace)
T = (0x8000, 0x8400)                                      # a temporary
PERSISTENT = [(0x1000, 0x4000)]


def check(*events, alive=PERSISTENT):
    return so.check(so.Trace(events, alive_start=alive, main=MAIN))


def kinds(rep):
    return sorted(v.split(":")[0] for v in rep.violations)


# ---------------------------------------------------------------------------------------------------------------------
# must be flagged
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_wait_before_a_side_stream_read():
    rep = check(so.access("gemm", MAIN, writes={"out": W}),
                so.record("e", MAIN),                                        # recorded, but the lane never waits for it
                so.access("colsum", LANE, reads={"x": W}))
    assert kinds(rep) == ["A RAW"] and not rep.unresolved
    text = rep.violations[0]
    for part in ("gemm#0(out, stream 0x0)", "colsum#0(x, stream 0x1)", "[0x1000, 0x2000)"):     # both calls, arguments, streams, bytes
        assert part in text, text


def test_side_stream_read_overwritten_by_the_main_stream():
    rep = check(so.access("gemm", MAIN, writes={"out": W}),
                so.record("e", MAIN), so.wait_event(LANE, "e"),
                so.access("colsum", LANE, reads={"x": W}),
                so.access("gemm", MAIN, writes={"out": W}))                  # no join in front of the second write
    assert kinds(rep) == ["A WAR"]
    assert "gemm#1(out, stream 0x0)" in rep.violations[0] and "colsum#0(x, stream 0x1)" in rep.violations[0]


def test_two_writers_with_no_edge():
    rep = check(so.access("colsum", MAIN, writes={"out": W}), so.access("colsum", LANE, writes={"out": (0x1800, 0x2800)}),
                alive=[(0x1000, 0x4000)])
    assert kinds(rep) == ["A WAW"] and "[0x1800, 0x2000)" in rep.violations[0]                   # the overlap, not either argument


def test_wait_on_an_event_recorded_again_after_the_wait():
    rep = check(so.record("e", MAIN), so.wait_event(LANE, "e"),
                so.access("gemm", MAIN, writes={"out": W}),
                so.record("e", MAIN),                                        # the record the lane needed: after its wait
                so.access("colsum", LANE, reads={"x": W}))
    assert kinds(rep) == ["A RAW"]


def test_wait_on_an_event_never_recorded():
    rep = check(so.access("gemm", MAIN, writes={"out": W}), so.wait_event(LANE, "never"), so.access("colsum", LANE, reads={"x": W}))
    assert kinds(rep) == ["A RAW"]


def test_temporary_of_the_main_stream_read_on_the_lane_without_record_stream():
    events = [so.alloc(MAIN, *T), so.access("gemm", MAIN, writes={"out": T}),
              so.record("e", MAIN), so.wait_event(LANE, "e"), so.access("colsum", LANE, reads={"x": T})]
    rep = check(*events)
    assert kinds(rep) == ["B lifetime"]
    assert "colsum#0(x, stream 0x1)" in rep.violations[0] and "[0x8000, 0x8400)" in rep.violations[0]
    assert check(*events, so.record_stream(*T, LANE)).clean()
    assert kinds(check(*events, so.record_stream(*T, THIRD))) == ["B lifetime"]                  # told about another stream
    # the same bytes, older than the trace and gone at its end: not persistent either
    rep = so.check(so.Trace(events[1:], alive_start=PERSISTENT + [T], alive_end=PERSISTENT, main=MAIN))
    assert kinds(rep) == ["B lifetime"]
    assert so.check(so.Trace(events[1:], alive_start=PERSISTENT + [T], main=MAIN)).clean()        # ... and alive at both ends


def test_unresolved_accesses_are_reported():
    ev = so.access("gemm", MAIN, writes={"out": W})
    ev[5].append("argument tables is a Mystery: not followed")
    rep = check(ev)
    assert not rep.violations and len(rep.unresolved) == 1 and "gemm#0" in rep.unresolved[0] and not rep.clean()


# ---------------------------------------------------------------------------------------------------------------------
# must pass clean
# ---------------------------------------------------------------------------------------------------------------------
def test_transitive_edge_through_a_third_stream():
    rep = check(so.access("gemm", MAIN, writes={"out": W}),
                so.record("a", MAIN), so.wait_event(THIRD, "a"),
                so.record("b", THIRD), so.wait_event(LANE, "b"),
                so.access("colsum", LANE, reads={"x": W}))
    assert rep.clean() and rep.pairs == 1


def test_join_by_wait_stream():
    events = [so.access("gemm", MAIN, writes={"out": W}),
              so.record("e", MAIN), so.wait_event(LANE, "e"),
              so.access("colsum", LANE, reads={"x": W}, writes={"out": (0x2000, 0x2100)}),
              so.wait_stream(MAIN, LANE),
              so.access("gemm", MAIN, reads={"x": (0x2000, 0x2100)}, writes={"out": W})]
    assert check(*events).clean()
    assert kinds(check(*(e for e in events if e[0] != "wait_stream"))) == ["A RAW", "A WAR"]     # ... which is what orders them


def test_disjoint_byte_ranges_of_one_tensor():
    assert check(so.access("gemm", MAIN, writes={"out": (0x1000, 0x1800)}), so.access("gemm", LANE, writes={"out": (0x1800, 0x2000)})).clean()


def test_fresh_allocation_where_another_stream_read_earlier():
    rep = check(so.alloc(MAIN, *T), so.access("gemm", MAIN, writes={"out": T}),
                so.record("e", MAIN), so.wait_event(LANE, "e"), so.access("colsum", LANE, reads={"x": T}),
                so.record_stream(*T, LANE),
                so.alloc(MAIN, *T),                                          # the allocator hands the block out again: its business
                so.access("gemm", MAIN, writes={"out": T}))
    assert rep.clean()


def test_same_stream_accesses():
    assert check(so.access("gemm", LANE, writes={"out": W}), so.access("colsum", LANE, reads={"x": W}),
                 so.access("gemm", LANE, writes={"out": W})).clean()


def test_two_streams_reading_the_same_weights():
    rep = check(so.access("gemm", MAIN, reads={"w": W}), so.access("gemm", LANE, reads={"w": W}), so.access("gemm", THIRD, reads={"w": W}))
    assert rep.clean() and rep.pairs == 0


def test_host_side_synchronize_orders_every_stream_behind_it():
    rep = check(so.access("gemm", LANE, writes={"out": W}), so.synchronize(), so.access("colsum", MAIN, reads={"x": W}),
                so.access("colsum", THIRD, reads={"x": W}))
    assert rep.clean()
    rep = check(so.access("gemm", LANE, writes={"out": W}), so.synchronize(("stream", THIRD)), so.access("colsum", MAIN, reads={"x": W}))
    assert kinds(rep) == ["A RAW"]


# ---------------------------------------------------------------------------------------------------------------------
# the write table
# ---------------------------------------------------------------------------------------------------------------------
def test_every_public_hip_function_is_classified():
    """Every public function of msclip_amd.hip is in WRITES (it takes tensors: what it writes) or in NO_TENSORS; the names in
    WRITES and EXTENTS are arguments the function has."""
    missing, bad = so.unclassified()
    assert not missing, f"classify in tests/stream_order.py (WRITES or NO_TENSORS): {missing}"
    assert not bad, bad
    stale = [n for n in list(so.WRITES) + list(so.NO_TENSORS) if n not in so.public_functions()]
    assert not stale, stale
    assert not set(so.WRITES) & set(so.NO_TENSORS)
    assert len(so.WRITES) >= 75                              # the launch-taking bindings of today


def test_a_wrapper_added_later_fails_until_classified(monkeypatch):
    def shiny_new_kernel(x, out):
        return out
    shiny_new_kernel.__module__ = hip.__name__
    monkeypatch.setattr(hip, "shiny_new_kernel", shiny_new_kernel, raising=False)
    assert so.unclassified() == (["shiny_new_kernel"], [])
    monkeypatch.setitem(so.WRITES, "shiny_new_kernel", ("out", "nope"))
    assert so.unclassified() == ([], ["shiny_new_kernel: nope"])


def test_write_paths():
    assert so.is_write("gemm", "out") and so.is_write("gemm", "fold_out.xb") and not so.is_write("gemm", "fold_out.center")
    assert not so.is_write("gemm", "x") and not so.is_write("gemm", "fold_in.rowstat")
    assert so.is_write("bn_bwd_fused", "sides.1.4") and not so.is_write("bn_bwd_fused", "sides.1.0")
    assert so.is_write("grad_accumulate", "accs.3") and not so.is_write("grad_accumulate", "grads.3")
    assert so.is_write("colsum", "return") and so.is_write("layernorm_bwd", "return.0") and not so.is_write("attention", "return")


def test_interval_follows_shape_and_stride():
    import torch
    t = torch.zeros(8, 16, dtype=torch.bfloat16)
    lo = t.data_ptr()
    assert so.interval(t) == (lo, lo + 256) and so.interval(t[2:4]) == (lo + 64, lo + 128)
    assert so.interval(t[:, 4:8]) == (lo + 8, lo + 7 * 32 + 16) and so.interval(t[:0]) is None
    out, unresolved = [], []
    so.walk(dict(a=[t, (t[1], None, 3)], f=hip.FoldIn(t[2], t[3]), odd=object()), "arg", out, unresolved)
    assert [p for p, _ in out] == ["arg.a.0", "arg.a.1.0", "arg.f.rowstat", "arg.f.csum"] and len(unresolved) == 1


def test_extent_functions_follow_the_call():
    """The row ranges of stream_order.EXTENTS: the token scatter of Engine._tokenise stays inside the image rows, the text front
    starts at row_base; a launch whose rows cannot be told from its arguments keeps the whole tensor."""
    import torch
    X = torch.zeros(400, 8)
    x = torch.zeros(196, 8)
    args = dict(x=x, M=4 * 49, conv=None, ldo=None, rpg=49, radd=1, roff=1, bn_stats_part=None)
    part = so.EXTENTS["gemm"]["out"](X, args)
    assert so.interval(part) == so.interval(X[1:200])                        # rows b * 50 + 1 + p, b < 4, p < 49
    assert so.interval(so.EXTENTS["gemm"]["out"](X, dict(args, M=None, rpg=hip.INT_MAX, radd=0, roff=0))) == so.interval(X[:196])
    assert so.EXTENTS["gemm"]["out"](X, dict(args, ldo=16)) is None          # a column window: rows of another stride
    assert so.EXTENTS["gemm"]["out"](X, dict(args, M=None, conv=(1,) * 7)) is None
    assert so.EXTENTS["gemm"]["out"](X, dict(args, M=500, rpg=hip.INT_MAX, radd=0, roff=0)) is None      # (not this tensor's rows)
    assert so.interval(so.EXTENTS["fill_cls"]["x"](X, dict(B=4, L=50))) == so.interval(X[:151])    # rows 0, 50, 100, 150
    part = so.EXTENTS["embed_tokens_packed"]["x"](X, dict(row_base=200, rows_padded=142))
    assert so.interval(part) == so.interval(X[200:342])
    tok = torch.zeros(2, 77, dtype=torch.int64)
    assert so.interval(so.EXTENTS["embed_tokens"]["x"](X, dict(row_base=200, tokens=tok))) == so.interval(X[200:354])
