"""The tracking restatements against the words they gave before their projection and word packing
were shared (tests/golden/track_words_golden.npz, written by tests/golden/gen_track_words.py): int64
words, compared exactly."""
import importlib.util
import os

import numpy as np

from conftest import GOLDEN


def test_restated_words_equal_the_golden():
    spec = importlib.util.spec_from_file_location("gen_track_words", os.path.join(GOLDEN, "gen_track_words.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    want = np.load(os.path.join(GOLDEN, "track_words_golden.npz"))
    got = gen.cases()
    assert sorted(got) == sorted(want.files) and len(got) == 13
    for name in want.files:
        assert got[name].dtype == np.int64 and got[name].shape == ((64,) if name.startswith("rgbd") else (32,)), name
        assert got[name].tolist() == want[name].tolist(), name
