"""generate(allowed_token_ids=A): the host-only half — normalisation and validation of A (`normalize_allowed_token_ids`) and
`evaluation.vocabulary_shortlist`.  No GPU."""
import numpy as np
import pytest
import torch

V = 1003


def _norm(a, **kw):
    from mic_amd.generation_clip_vision_utils import normalize_allowed_token_ids

    return normalize_allowed_token_ids(a, V, **kw)


def test_sorted_unique_int32_whatever_the_order_and_the_container():
    want = np.array([2, 5, 17, 996, 1002], dtype=np.int32)
    raw = [996, 5, 2, 17, 5, 1002, 2]
    for a in (raw, tuple(raw), np.array(raw), np.array(raw, dtype=np.int16), np.array(raw, dtype=np.uint64), torch.tensor(raw),
              torch.tensor(raw, dtype=torch.int32), [np.int64(v) for v in raw]):
        got = _norm(a)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.ndim == 1
        assert np.array_equal(got, want), a
    assert np.array_equal(_norm([7]), np.array([7], dtype=np.int32))  # one id is enough for a greedy search
    assert np.array_equal(_norm(list(range(V - 3, V))), np.arange(V - 3, V, dtype=np.int32))


@pytest.mark.parametrize("bad", [[], (), np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int64),           # empty
                                 [1.0, 2.0], np.array([1.0, 2.0]), torch.tensor([1.5]), [True, False], ["a"], [3, None],  # not integers
                                 np.array([[1, 2], [3, 4]]), torch.tensor([[1, 2]]), np.array(5), 5, None, "12", {1, 2},  # not 1-D sequences
                                 [-1, 4], [4, V], np.array([2 ** 40])])                                              # outside [0, V)
def test_malformed_sets_are_refused(bad):
    with pytest.raises(ValueError, match="allowed_token_ids"):
        _norm(bad)


def test_what_the_search_must_emit_has_to_be_listed():
    a = [2, 10, 11, 12, 13, 14, 15, 996]
    assert _norm(a, eos_token_id=2, forced_bos_token_id=996, forced_eos_token_id=2, num_beams=4).size == 8
    with pytest.raises(ValueError, match="eos_token_id"):
        _norm(a[1:], eos_token_id=2)
    with pytest.raises(ValueError, match="forced_bos_token_id"):
        _norm(a, eos_token_id=2, forced_bos_token_id=995)
    with pytest.raises(ValueError, match="forced_eos_token_id"):
        _norm(a, eos_token_id=2, forced_eos_token_id=3)
    with pytest.raises(ValueError, match="language id 995"):
        _norm(a, eos_token_id=2, language_bos_ids=[996, 995])
    assert _norm(a, eos_token_id=2, language_bos_ids=[996, 996]).size == 8
    # not in force = None: nothing to check (start ids and PAD are never asked about)
    assert _norm([5, 6], eos_token_id=None, forced_bos_token_id=None, forced_eos_token_id=None).size == 2


def test_beam_search_needs_two_candidates_per_beam():
    a = list(range(10, 18))  # 8 ids
    assert _norm(a, num_beams=4).size == 8
    assert _norm(a + a, num_beams=4).size == 8
    with pytest.raises(ValueError, match="num_beams=5"):
        _norm(a, num_beams=5)
    with pytest.raises(ValueError, match="num_beams=4"):
        _norm(a[:7] + a[:3], num_beams=4)  # duplicates do not count
    assert _norm([3], num_beams=1).size == 1


def test_sampling_is_refused():
    with pytest.raises(NotImplementedError, match="do_sample"):
        _norm([2, 3, 4], do_sample=True)
    with pytest.raises(ValueError):  # a malformed set is reported first
        _norm([], do_sample=True)


def test_vocabulary_shortlist():
    from mic_amd.evaluation import vocabulary_shortlist

    labels = [np.array([[996, 10, 11, 2, 1, 1], [996, 12, 10, 2, 1, 1]]), torch.tensor([995, 40, 41, 2]), [7, 7, 7], np.zeros((0, 4), dtype=np.int64)]
    got = vocabulary_shortlist(labels, always=(2, 994))
    assert got.dtype == np.int32 and got.ndim == 1
    assert got.tolist() == [1, 2, 7, 10, 11, 12, 40, 41, 994, 995, 996]
    assert vocabulary_shortlist(iter(labels[:1])).tolist() == [1, 2, 10, 11, 12, 996]  # any iterable
    assert vocabulary_shortlist([], always=[5, 3, 5]).tolist() == [3, 5]
    assert vocabulary_shortlist([]).size == 0
    with pytest.raises(ValueError):
        vocabulary_shortlist([np.array([1.0, 2.0])])
    with pytest.raises(ValueError):
        vocabulary_shortlist([np.array([-3, 4])])
    # what it returns is what generate() accepts
    assert np.array_equal(_norm(got, eos_token_id=2, language_bos_ids=[996, 995, 994], num_beams=4), got)
