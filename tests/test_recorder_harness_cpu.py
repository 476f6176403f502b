"""CPU tests of the recorder family's harness (tests/recorder.py, tests/recorder_rows.py): the parts the GPU suite can check only
indirectly -- that the comparisons pass on equal inputs and, on one changed value, fail with a message that says where; how
tfrec_gpu's lines are picked by their first word; and that no test module of the family imports another."""
import glob
import os
import re

import numpy as np
import pytest

import parity
import recorder as R
from parity import imports_of
from tfrec_amd import capture

DTYPES = {"run": capture.RUN_DTYPE, **{m: st.dtype for m, st in R.STAGES.items()}}


def records(dtype, n=5, seed=1):
    """n records whose every byte is drawn."""
    return np.random.default_rng(seed).integers(0, 256, n * dtype.itemsize, dtype=np.uint8).view(dtype).copy()


def message(f, *args):
    with pytest.raises(AssertionError) as e:
        f(*args)
    return str(e.value)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_same_records_passes_on_equal_arrays_and_names_the_record_and_field_that_differ(name):
    dtype = DTYPES[name]
    want = records(dtype)
    R.same_records(want.copy(), want, name)
    R.same_records(want[:0].copy(), want[:0], name)  # no records at all
    arrays = [f for f in dtype.names if dtype[f].shape]
    assert {"meter": "hist", "clock": "spec"}.get(name) in arrays + [None]  # the array fields: each is changed below, in one element
    for k, f in enumerate(dtype.names):
        got, i = want.copy(), k % len(want)
        if dtype[f].shape:
            got[f][i, -1] += 1  # one element of the record's array
        else:
            got[f][i] += 1
        text = message(R.same_records, got, want, "label-%s" % name)
        assert "label-%s" % name in text and "record %d " % i in text and "field %s:" % f in text, text
    assert "4 records, want 5" in message(R.same_records, want[:4], want, name)
    other = np.zeros(5, dtype=[("stream", "<u4")])
    assert "dtype" in message(R.same_records, other, want, name) and "dtype" in message(R.same_records, want, other, name)


def test_same_words_names_the_word_with_a_flipped_bit():
    want = np.arange(40, dtype=np.uint32) * 2654435761
    R.same_words(want.copy(), want)
    got = want.copy()
    got[17] ^= 1 << 9
    text = message(R.same_words, got, want, "bitmap")
    assert "bitmap" in text and "1 words differ, the first at 17:" in text and "%08x" % want[17] in text, text
    assert "39 words" in message(R.same_words, want[:39], want)
    assert "int32" in message(R.same_words, want.astype(np.int32), want)


@pytest.mark.parametrize("name", sorted(R.STAGES))
def test_same_table_takes_a_prefix_and_names_a_changed_field(name):
    runs = records(capture.RUN_DTYPE, 6, seed=2)
    recs = records(R.STAGES[name].dtype, 6, seed=3)
    for f in R.TABLE_FIELDS:
        recs[f] = runs[f]
    R.same_table(recs, runs, name)
    R.same_table(recs[:4], runs, name)  # a table longer than the records: the prefix an overflow delivers
    R.same_table(recs[:0], runs, name)
    assert "6 records repeat a table of 5 runs" in message(R.same_table, recs, runs[:5], name)
    for k, f in enumerate(R.TABLE_FIELDS):
        got = recs.copy()
        got[f][k] += 1
        text = message(R.same_table, got, runs, name)
        assert name in text and "record %d " % k in text and "field %s " % f in text, text
    if name in ("track", "sync"):  # table_of: what these two repeat of the table, pool_offset included
        t = R.table_of(recs)
        assert t.dtype == capture.RUN_DTYPE and all(np.array_equal(t[f], runs[f]) for f in R.TABLE_FIELDS)
        assert np.array_equal(t["pool_offset"], recs["bit_offset"])


def test_pick_takes_a_line_by_its_first_word():
    text = "burst a\nbursty b\nextent c\n\nTFA2 ID 7a +21.3 60 0 0 RSSI 80 Offset 1kHz\n burst d\nframe e\nburst f g\n"
    got = R.pick(text, "burst", "extent", "clock", ("frame", "burst"))
    assert got["burst"] == ["burst a", "burst f g"] and got["extent"] == ["extent c"] and got["clock"] == []
    assert got[("frame", "burst")] == ["burst a", "frame e", "burst f g"]  # either word, in the order of the output
    assert got["telegrams"] == parity.telegram_lines(text) == ["TFA2 ID 7a +21.3 60 0 0 RSSI 80 Offset 1kHz"]
    assert R.pick(text, "burst")["burst"] == got["burst"] and sorted(R.pick(text, "burst"), key=str) == ["burst", "telegrams"]
    assert R.pick("", "burst") == {"burst": [], "telegrams": []}
    words = [st.word for st in R.STAGES.values()]  # the five stages' lines: no word takes another's
    assert words == ["burst", "extent", "clock", "bits", "frame"]
    got = R.pick("".join("%s f %d\n" % (w, k) for k, w in enumerate(words)), *words)
    assert [got[w] for w in words] == [["%s f %d" % (w, k)] for k, w in enumerate(words)]


# ---- the import rule
HERE = os.path.dirname(os.path.abspath(__file__))
FAMILY = re.compile(r"test_((capture|burst|envelope|clock|track|sync|decin)_(gpu|cpu)|recorder_campaign_(gpu|cpu))$")


def test_no_module_imports_a_test_module_of_the_family_and_the_harness_imports_no_test_module():
    paths = sorted(glob.glob(os.path.join(HERE, "*.py")))
    assert len(paths) > 50 and {"recorder.py", "recorder_rows.py", "recorder_campaign.py"} <= {os.path.basename(p) for p in paths}
    assert sum(1 for p in paths if FAMILY.match(os.path.basename(p)[:-3])) == 16
    for p in paths:
        name, found = os.path.basename(p), imports_of(p)
        assert not [m for m in found if FAMILY.match(m)], "%s imports %s" % (name, sorted(m for m in found if FAMILY.match(m)))
        if name in ("recorder.py", "recorder_rows.py", "recorder_campaign.py"):
            assert not [m for m in found if m.startswith("test_")], "%s imports %s" % (name, sorted(found))
    assert "meter_rows" in imports_of(os.path.join(HERE, "test_capture_cpu.py"))  # (imports_of sees `from m import n`)
    assert "recorder_rows" in imports_of(os.path.join(HERE, "test_recorder_campaign_cpu.py"))  # ... and one inside a function
