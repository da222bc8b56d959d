"""Random-forest classification, the parts that need no GPU: forest import (arrays, sklearn,
.npz), the library's forest check, the rfrawp column of the segment table and the Arrow join.
The device inference itself is tests/test_gpu_randomforest.py."""
import ctypes
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import ccdgpu
import forest_util
from ccdgpu import abi
from ccdc import randomforest, segment, sink
from ccdc.randomforest import Forest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sk_forest(labels, n_trees=7, max_depth=5, n_features=6, n=600, seed=0):
    from sklearn.ensemble import RandomForestClassifier
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, n_features)).astype(np.float32)
    y = np.asarray(labels)[rng.integers(0, len(labels), n)]
    rf = RandomForestClassifier(n_estimators=n_trees, max_depth=max_depth, random_state=seed, n_jobs=1).fit(x, y)
    return rf, x


def test_from_sklearn_walk_matches_predict_proba():
    rf, x = _sk_forest([0, 1, 2, 3])
    f = Forest.from_sklearn(rf)
    assert (f.n_trees, f.n_features, f.n_classes) == (7, 6, 4)
    assert f.max_depth <= 5
    np.testing.assert_allclose(f.value[f.feature < 0].sum(axis=1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(forest_util.walk_raw(f, x) / f.n_trees, rf.predict_proba(x), rtol=0, atol=1e-12)


def test_from_sklearn_label_gaps_become_zero_columns():
    rf, x = _sk_forest([0, 1, 3, 8])
    f = Forest.from_sklearn(rf)
    assert f.n_classes == 9
    raw = forest_util.walk(f, x)
    assert raw.shape == (x.shape[0], 9)
    assert not raw[:, [2, 4, 5, 6, 7]].any()
    np.testing.assert_allclose(raw[:, [0, 1, 3, 8]].astype(np.float64) / f.n_trees, rf.predict_proba(x), rtol=0, atol=1e-6)


@pytest.mark.parametrize('labels', [[-1, 0, 1], [0.5, 1.0], ['a', 'b'], [0, 40]])
def test_from_sklearn_rejects_labels_spark_cannot_index(labels):
    if isinstance(labels[0], float):  # (sklearn itself refuses to fit fractional labels)
        rf, _ = _sk_forest(list(range(len(labels))))
        rf.classes_ = np.asarray(labels)
    else:
        rf, _ = _sk_forest(labels)
    with pytest.raises(ValueError):
        Forest.from_sklearn(rf)


def _small():
    #        0
    #      1   4
    #     2 3
    return dict(root=[0], feature=[0, 1, -1, -1, -1], threshold=[0.5, -1.0, 0, 0, 0], left=[1, 2, -1, -1, -1],
                right=[4, 3, -1, -1, -1], value=[[0, 0], [0, 0], [1, 0], [0.5, 0.5], [0, 1]], n_features=2)


MALFORMED = {
    'n_features above the limit': (dict(n_features=65), 'n_features'),
    'n_features zero': (dict(n_features=0), 'n_features'),
    'n_classes above the limit': (dict(value=np.zeros((5, 33))), 'n_classes'),
    'no trees': (dict(root=[]), 'n_trees'),
    'root out of range': (dict(root=[5]), 'root'),
    'root negative': (dict(root=[-1]), 'root'),
    'child out of range': (dict(right=[9, 3, -1, -1, -1]), 'right child of node 0'),
    'child negative': (dict(left=[1, -2, -1, -1, -1]), 'left child of node 1'),
    'child not greater than parent': (dict(left=[1, 1, -1, -1, -1]), 'not greater'),
    'child equal to an ancestor': (dict(right=[4, 0, -1, -1, -1]), 'not greater'),
    'feature out of range': (dict(feature=[0, 2, -1, -1, -1]), 'feature 2'),
    'threshold nan': (dict(threshold=[np.nan, -1.0, 0, 0, 0]), 'non-finite threshold'),
    'threshold inf': (dict(threshold=[0.5, np.inf, 0, 0, 0]), 'non-finite threshold'),
    'leaf value nan': (dict(value=[[0, 0], [0, 0], [1, 0], [np.nan, 0.5], [0, 1]]), 'non-finite value'),
    'leaf value inf': (dict(value=[[0, 0], [0, 0], [1, 0], [0.5, 0.5], [0, np.inf]]), 'non-finite value'),
    'node with two parents': (dict(right=[4, 2, -1, -1, -1]), 'two parents'),
}


@pytest.mark.parametrize('case', sorted(MALFORMED))
def test_forest_check_rejects(case):
    change, word = MALFORMED[case]
    a = dict(_small(), **change)
    with pytest.raises(ValueError, match=re.escape(word)):
        Forest.from_arrays(**a)
    f, keep = abi.forest_struct(**a)
    assert ccdgpu.lib().ccdgpu_forest_check(ctypes.byref(f)) == abi.E_INVAL
    assert word in ccdgpu.last_error()


def test_forest_check_accepts_the_small_tree_and_a_single_leaf():
    f = Forest.from_arrays(**_small())
    assert f.max_depth == 2
    leaf = Forest.from_arrays(root=[0], feature=[-1], threshold=[0.0], left=[-1], right=[-1], value=[[0.25, 0.75]],
                              n_features=1)
    assert leaf.max_depth == 0 and leaf.n_classes == 2
    # a non-finite threshold or value the walk never reads is no error: leaves' thresholds,
    # internal nodes' values
    a = _small()
    a['threshold'][2] = np.nan
    a['value'][0] = [np.inf, np.nan]
    Forest.from_arrays(**a)
    np.testing.assert_array_equal(forest_util.walk(leaf, np.zeros((3, 1))), np.tile(np.float32([0.25, 0.75]), (3, 1)))


def test_forest_depth_of_generated_forests():
    assert Forest.from_arrays(*forest_util.random_forest(1, 3, 6, 4, 3, p_leaf=0.0).args()).max_depth == 6
    assert Forest.from_arrays(*forest_util.random_forest(2, 5, 0, 4, 3).args()).max_depth == 0


def test_save_load_round_trip(tmp_path):
    f = Forest.from_arrays(*forest_util.random_forest(3, 4, 5, 33, 9).args())
    path = str(tmp_path / 'forest.npz')
    f.save(path)
    g = Forest.load(path)
    assert g.n_features == f.n_features
    for k in forest_util.ARRAYS:
        a, b = getattr(f, k), getattr(g, k)
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(a, b)


def _rows(n=5):
    rows = np.zeros(n, dtype=abi.ROW_DTYPE)
    rng = np.random.default_rng(5)
    rows['px'] = 100 + 30 * (np.arange(n) // 2)
    rows['py'] = 200
    rows['sday'] = 724000 + 400 * np.arange(n)
    rows['eday'] = rows['sday'] + 300
    rows['bday'] = rows['eday'] + 16
    rows['has_model'] = 1
    rows['curqa'] = 8
    rows['chprob'] = 1.0
    for k in ('mag', 'rmse', 'coef', 'intercept'):
        rows[k] = rng.normal(size=rows[k].shape)
    rows[3]['has_model'] = 0  # pyccd.default's row
    rows[3]['sday'] = rows[3]['eday'] = rows[3]['bday'] = 1
    return rows


def test_segment_table_fills_rfrawp_and_nulls_nan_rows():
    rows = _rows()
    raw = np.random.default_rng(1).random((5, 9)).astype(np.float32)
    raw[3] = np.nan
    t = sink.segment_table(10, 20, rows, rfrawp=raw)
    assert t.schema == sink.arrow_schema(segment.schema())
    got = t['rfrawp'].to_pylist()
    assert got[3] is None
    for i in (0, 1, 2, 4):
        assert np.float32(got[i]).tolist() == raw[i].tolist()
    off = np.array([0, 2, 4, 5])
    mask = np.zeros((3, 4), dtype=np.int8)
    tabs = sink.tables(10, 20, np.arange(4) + 730000, off, rows, mask, rfrawp=raw)
    assert tabs['segment'].equals(t)
    with pytest.raises(ValueError):
        sink.segment_table(10, 20, rows, rfrawp=raw[:4])


def test_segment_table_without_rfrawp_is_unchanged():
    rows = _rows()
    t = sink.segment_table(10, 20, rows)
    cols = sink._row_columns(10, 20, rows)
    cols['rfrawp'] = pa.nulls(rows.shape[0], type=pa.list_(pa.float32()))  # the column as it was written so far
    schema = sink.arrow_schema(segment.schema())
    was = pa.table([cols[f.name] for f in schema], schema=schema)
    assert t.equals(was)
    assert t.equals(sink.segment_table(10, 20, rows, rfrawp=None))
    assert t['rfrawp'].null_count == rows.shape[0]
    off, mask = np.array([0, 2, 4, 5]), np.zeros((3, 4), dtype=np.int8)
    assert sink.tables(10, 20, np.arange(4) + 730000, off, rows, mask)['segment'].equals(t)


def test_join_is_segment_joins_contract():
    """segment.join: inner on (cx, cy, px, py, sday, eday), the segments' own rfrawp dropped for
    the predictions' -- on 5 rows, one without a prediction, predictions in another order, and a
    prediction that matches no segment."""
    seg = sink.segment_table(10, 20, _rows())
    keys = {k: seg[k].to_pylist() for k in randomforest.KEYS}
    order = [4, 0, 2, 1]  # (row 3, pyccd.default's, has no prediction)
    raw = [[float(i), 0.5] for i in order]
    pred = {k: [keys[k][i] for i in order] + [keys[k][0]] for k in randomforest.KEYS}
    pred['sday'][-1] = '1999-01-01'  # no such segment
    pred = pa.table(dict(pred, rfrawp=pa.array(raw + [[9.0, 9.0]], type=pa.list_(pa.float32()))))
    j = randomforest.join(seg, pred)
    assert j.schema == seg.schema
    assert j.num_rows == 4
    assert j['sday'].to_pylist() == [keys['sday'][i] for i in (0, 1, 2, 4)]
    assert j['rfrawp'].to_pylist() == [[0.0, 0.5], [1.0, 0.5], [2.0, 0.5], [4.0, 0.5]]
    for name in seg.column_names:
        if name != 'rfrawp':
            assert j[name].to_pylist() == [seg[name].to_pylist()[i] for i in (0, 1, 2, 4)], name


def test_abi_struct_sizes_match_the_header():
    txt = open(os.path.join(ROOT, 'include', 'ccdgpu.h')).read()
    assert int(re.search(r'#define CCDGPU_FOREST_MAX_FEATURES (\d+)', txt).group(1)) == abi.FOREST_MAX_FEATURES == 64
    assert int(re.search(r'#define CCDGPU_FOREST_MAX_CLASSES (\d+)', txt).group(1)) == abi.FOREST_MAX_CLASSES == 32
    body = txt[txt.index('typedef struct ccdgpu_forest {'):txt.index('} ccdgpu_forest;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in re.findall(r'([^;{]+);', body) for n in re.findall(r'\*?(\w+)\s*(?:,|$)', decl.strip())]
    assert names == [n for n, _ in abi.Forest._fields_]
    assert ctypes.sizeof(abi.Forest) == 4 * 4 + 6 * ctypes.sizeof(ctypes.c_void_p) == 64
    for n in ('root', 'feature', 'left', 'right'):
        assert dict(abi.Forest._fields_)[n] == ctypes.POINTER(ctypes.c_int32)
    for n in ('threshold', 'value'):
        assert dict(abi.Forest._fields_)[n] == ctypes.POINTER(ctypes.c_double)
    for name in ('ccdgpu_forest_check', 'ccdgpu_forest_depth', 'ccdgpu_forest_set', 'ccdgpu_forest_clear',
                 'ccdgpu_classify', 'ccdgpu_classify_rows'):
        assert name in ccdgpu.EXPORTS and hasattr(ccdgpu.lib(), name)
