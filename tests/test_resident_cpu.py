"""The host half of the resident training split (facl_amd/resident.py) without a GPU: the header pass and the table builder
are pure NumPy, the budget arithmetic is plain integers, the entry's flag validation comes before any device call, and the
new C entries refuse null pointers and bad sizes before any launch."""
import os

import numpy as np
import pytest

from synth_tree import clip_names, write_clip


def _clip(seed, sizes, dt=np.float64):
    r = np.random.RandomState(seed)
    arrs = [r.rand(n, 8) - 0.5 for n in sizes]
    arrs[0][0, 4] = arrs[0][0, 7] = 0.25
    return tuple(a.astype(dt) for a in arrs)


def _sizes(i):
    return (600 + 7 * i, 300 + 3 * i, 400 + 5 * i, 150 + i)


def _tree(root, n=9, dt=np.float64):
    from facl_amd.dataset import ClipIndex
    names = clip_names(n)
    for i, nm in enumerate(names):
        write_clip(root, nm, _clip(i, _sizes(i), dt))
    return ClipIndex.from_dir(os.path.join(str(root), "reslution", "Resolution60", "raw"), "ntu120")


def test_header_pass_and_table_give_exact_totals_and_offsets(tmp_path):
    from facl_amd import resident as R
    index = _tree(tmp_path)
    split = index.select("view")                                    # cameras 2 and 3: 6 of the 9 clips
    assert len(split) == 6
    rows, dt = R.header_pass(index, str(tmp_path), "0", split)
    assert dt == np.float64 and rows.dtype == np.int64
    want = np.array([_sizes(clip_names(9).index(index.names[v][:20])) for v in split], dtype=np.int64)
    np.testing.assert_array_equal(rows, want)
    table, rows_total, rows0_total = R.build_table(rows, split)
    assert table.dtype == np.int64 and table.shape == (6, R.REC)
    assert rows_total == int(want.sum()) and rows0_total == int(want[:, 0].sum())
    off = 0
    for i in range(6):
        for k in range(4):
            assert table[i, k] == off and table[i, 4 + k] == want[i, k]
            off += int(want[i, k])
        assert table[i, 8] == split[i] and table[i, 9] == int(want[:i, 0].sum())
        assert table[i, 10] == 0 and table[i, 11] == 0
    b = R.pool_bytes(rows, dt.itemsize)
    assert b == {"src": rows_total * 8 * 8, "lists": 2 * rows0_total * 4, "table": 6 * R.REC * 8,
                 "total": rows_total * 64 + rows0_total * 8 + 6 * R.REC * 8}
    assert R.pool_bytes(rows, 4)["src"] == rows_total * 8 * 4


def test_offsets_stay_exact_past_two_to_the_31_rows():
    from facl_amd import resident as R
    n = 80000                                                        # 80,000 clips of 4 x 8,192 rows: 2.6e9 rows
    rows = np.full((n, 4), 8192, dtype=np.int64)
    rows[::7, 0] = 8191
    table, rows_total, rows0_total = R.build_table(rows, np.arange(n))
    assert rows_total == int(rows.sum()) > 1 << 31
    assert table.dtype == np.int64 and int(table[-1, 3]) > 1 << 31
    flat = [int(x) for x in rows.reshape(-1)]                        # Python integers: no wrap possible
    acc, i = 0, 0
    for j in (0, 1, 65535, 65536, 65537, n - 1):                     # around the 2^31-row mark and at the ends
        while i < 4 * j:
            acc += flat[i]
            i += 1
        assert [int(x) for x in table[j, :4]] == [acc, acc + flat[i], acc + flat[i] + flat[i + 1],
                                                  acc + flat[i] + flat[i + 1] + flat[i + 2]]
    assert int(table[-1, 3]) + 8192 == rows_total
    assert int(table[-1, 9]) + int(rows[-1, 0]) == rows0_total
    assert R.pool_bytes(rows, 8)["src"] == rows_total * 64
    with pytest.raises(ValueError):
        R.build_table([[1 << 30, 1 << 30, 1, 1]], [0])               # a clip's rows must stay clip-relative int32
    with pytest.raises(ValueError):
        R.build_table([[5, 0, 1, 1]], [0])


def test_header_pass_refuses_what_load_clip_refuses(tmp_path):
    from facl_amd import resident as R
    index = _tree(tmp_path / "a", n=6)
    split = index.select("view")
    nm = index.v_name(split[1])
    write_clip(tmp_path / "a", nm, _clip(50, (10, 10, 10, 10), np.float32))
    with pytest.raises(ValueError, match="mixes float32 and float64.*" + nm):
        R.header_pass(index, str(tmp_path / "a"), "0", split)
    c = list(_clip(51, (10, 10, 10, 10)))
    c[2] = c[2][:, :7]
    write_clip(tmp_path / "a", nm, c)
    with pytest.raises(ValueError, match=nm + ".*rows, >=8"):
        R.header_pass(index, str(tmp_path / "a"), "0", split)
    c = list(_clip(52, (10, 10, 10, 10)))
    c[1] = c[1].astype(np.float32)
    write_clip(tmp_path / "a", nm, c)
    with pytest.raises(ValueError, match="share one dtype"):
        R.header_pass(index, str(tmp_path / "a"), "0", split)
    with pytest.raises(ValueError, match="3-D"):
        R.check_clip_shapes("x", [(4, 10, 8), (10, 8), (10, 8), (10, 8)], [np.dtype(np.float64)] * 4, "1")


def test_budget_refuses_and_accepts_at_the_boundary():
    from facl_amd import resident as R
    gib = 1 << 30
    R.check_budget(2 * gib, free=0, max_gb=2.0)                      # need == bound: accepted (free memory is not consulted)
    with pytest.raises(RuntimeError, match=str(2 * gib + 1)):
        R.check_budget(2 * gib + 1, free=100 * gib, max_gb=2.0)
    R.check_budget(10 * gib, free=10 * gib + 512, max_gb=0, reserve=512)
    with pytest.raises(RuntimeError) as e:
        R.check_budget(10 * gib + 1, free=10 * gib + 512, max_gb=0, reserve=512)
    for figure in (10 * gib + 1, 10 * gib + 512, 512):               # the need, the free memory and the reserve
        assert str(figure) in str(e.value)
    assert R.STEP_RESERVE_BYTES == 2 * R.STEP_PEAK_BYTES


def test_chunks_cover_the_split_in_order():
    from facl_amd import resident as R
    rows = np.array([_sizes(i) for i in range(11)], dtype=np.int64)
    for kw in ({"chunk_clips": 1}, {"chunk_clips": 5}, {"chunk_clips": 11}, {"chunk_clips": 100}, {},
               {"staging_bytes": 1}, {"staging_bytes": 3 * 1500 * 64}):
        ch = R.chunk_ranges(rows, 8, **kw)
        assert ch[0][0] == 0 and ch[-1][1] == 11
        assert all(a < b for a, b in ch) and all(ch[i][1] == ch[i + 1][0] for i in range(len(ch) - 1))
    assert len(R.chunk_ranges(rows, 8, staging_bytes=1)) == 11
    assert R.chunk_ranges(rows, 8, chunk_clips=5) == [(0, 5), (5, 10), (10, 11)]
    assert R.MAX_WORKERS == 16


@pytest.mark.parametrize("extra, reason", [(["--synthetic", "1", "--view_rng", "philox"], "needs --synthetic 0"),
                                           (["--synthetic", "0", "--view_rng", "numpy"], "on the host")])
def test_entry_refuses_resident_with_the_wrong_mode_before_any_device_call(tmp_path, monkeypatch, extra, reason):
    import torch
    from facl_amd import cn3d_train_motion_GL as train

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the flags were checked")
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    with pytest.raises(RuntimeError, match=reason):
        train.main(["--resident", "1", "--data_root", str(tmp_path), "--save_root_dir", str(tmp_path / "ck")] + extra)


def test_new_entries_refuse_null_pointers_and_bad_sizes_before_any_launch():
    from facl_amd import _lib, build
    build.build()
    lib = _lib.load_library()
    p = 4096                                                          # never dereferenced: every call is refused on the host
    E_SHAPE, E_NULL, E_ALIGN = -1, -2, -3
    for sfx in ("f32", "f64"):
        rows = getattr(lib, "facl_resident_temporal_rows_" + sfx)
        for bad in range(4):
            a = [p, p, p, p]
            a[bad] = None
            assert rows(a[0], a[1], a[2], 0, 1, a[3], None) == E_NULL
        assert rows(p, p, p, 0, 0, p, None) == E_SHAPE
        assert rows(p, p, p, -1, 1, p, None) == E_SHAPE
        assert rows(p, p, p, 2 ** 31 - 1, 1, p, None) == E_SHAPE
        views = getattr(lib, "facl_build_views_resident_" + sfx)
        good = dict(src=p, table=p, lists=p, n=4, sel=p, B=2, out=p, idx=None, err=p)

        def call(**kw):
            g = dict(good, **kw)
            return views(g["src"], g["table"], g["lists"], g["n"], g["sel"], g["B"], 1, 0, g["out"], g["idx"], g["err"], None)
        for k in ("src", "table", "lists", "sel", "out", "err"):
            assert call(**{k: None}) == E_NULL
        assert call(n=0) == E_SHAPE and call(B=0) == E_SHAPE and call(B=(1 << 20) + 1) == E_SHAPE
        assert call(out=p + 8) == E_ALIGN
