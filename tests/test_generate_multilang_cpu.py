"""generate() with a sequence of language ids, the parts that need no device: the argument normaliser and the two C-ABI entry
points the grouped decode chain adds (binding table and header)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _norm(*a, **kw):
    import mic_amd  # noqa: F401
    from mic_amd.generation_clip_vision_utils import normalize_language_ids

    return normalize_language_ids(*a, **kw)


def test_scalars_stay_ungrouped():
    assert _norm(None, None) == (1, None, None, False)
    assert _norm(999, None) == (1, None, [999], False)
    assert _norm(None, 996) == (1, [996], None, False)
    assert _norm(decoder_start_token_id=np.int64(7), forced_bos_token_id=np.array(5)) == (1, [5], [7], False)  # 0-d array: a scalar


@pytest.mark.parametrize("make", [list, tuple, lambda v: np.array(v, dtype=np.int64), lambda v: np.array(v, dtype=np.int32),
                                  lambda v: torch.tensor(v, dtype=torch.int64), lambda v: torch.tensor(v, dtype=torch.int32)])
@pytest.mark.parametrize("ids", [[996, 995, 994, 993], [996]])
def test_sequences_are_grouped_whatever_their_length(make, ids):
    G, bos, start, grouped = _norm(None, make(ids))
    assert (G, bos, start, grouped) == (len(ids), ids, None, True)
    assert all(type(v) is int for v in bos)
    G, bos, start, grouped = _norm(make(ids), None)
    assert (G, bos, start, grouped) == (len(ids), None, ids, True)


def test_scalar_beside_a_sequence_is_broadcast():
    assert _norm(999, [996, 995, 994]) == (3, [996, 995, 994], [999, 999, 999], True)
    assert _norm((999, 998), np.int32(996)) == (2, [996, 996], [999, 998], True)
    assert _norm([999, 998], [996, 995]) == (2, [996, 995], [999, 998], True)
    assert _norm([999], 996) == (1, [996], [999], True)


@pytest.mark.parametrize("args", [([999, 998], [996, 995, 994]), ([], None), (None, ()), (None, np.array([], dtype=np.int64)),
                                  (None, [996, 995.0]), (None, [996, "995"]), (None, np.array([996.0, 995.0])), (None, [996, True]),
                                  (None, np.array([[996, 995]])), (None, [996, None]), (999.5, [996, 995]), ("en", [996])])
def test_bad_language_arguments_raise_value_error(args):
    with pytest.raises(ValueError):
        _norm(*args)


def test_new_entry_points_are_bound_and_declared():
    import mic_amd  # noqa: F401
    from mic_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "mic_hip.h")).read()
    for name in ("mic_row_forced_topk", "mic_beam_step_groups"):
        assert name in _lib.EXPORTS
        assert re.search(rf"^int\s+{name}\s*\(", hdr, flags=re.M), f"{name} is not declared in include/mic_hip.h"
        assert hasattr(_lib.lib(), name)
    # the reference lines the two serve are named beside their declarations
    doc = hdr[hdr.index("mic_row_forced_topk:"): hdr.index("int mic_beam_step_groups")]
    assert "gen:412-419" in doc and "gen:798-820" in doc


def test_generate_languages_rejects_an_unknown_selector():
    import mic_amd  # noqa: F401
    from mic_amd.evaluation import generate_languages

    with pytest.raises(ValueError):
        generate_languages(None, None, {"en_XX": 996}, via="bos")
