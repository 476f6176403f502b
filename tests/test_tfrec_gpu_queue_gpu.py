"""tfrec_gpu -n: a queue of dump files through a fixed number of streams per device (tfrec_amd_reset_streams recycles a
stream when its file has ended).  Every file's records, -m 1 summary and -q output equal those of running that file alone;
with at least one stream per file the output is byte for byte that of a run without -n.  -B (BITS replay) checks that the
BITS chunks of a file in a recycled stream count their samples from the file's start, like its flushes: the engine cuts
and orders both by end_sample."""
import pytest

import parity
from tfrec_amd import synth

pytestmark = pytest.mark.gpu

BLOCKS = (5, 9, 3, 8, 6)  # blocks per dump: some not a multiple of -b 4


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    parity.build_cli()
    d = tmp_path_factory.mktemp("dumps")
    files = []
    for k, nb in enumerate(BLOCKS):
        p = d / ("f%d.iq" % k)
        iq = synth.gen_stream(61, k, nb)
        # (file 1 ends in a partial block: dropped, as by the reference)
        p.write_bytes(iq.tobytes() + (b"\x80" * 1000 if k == 1 else b""))
        files.append(str(p))
    return d, files


def run(args, files, sink):
    return parity.cli(["-T", "2f", "-t", "500", "-b", "4"] + args + sum((["-L", f] for f in files), []), sink)


@pytest.mark.parametrize("extra", [[], ["-m", "1"], ["-q"], ["-B"]], ids=["default", "summary", "quiet", "bits"])
def test_each_file_through_two_streams_equals_the_file_alone(dumps, extra):
    d, files = dumps
    _, recs = run(["-n", "2"] + extra, files, d / "q.out")
    assert {r[0] for r in recs} == {str(k) for k in range(len(files))}
    n = 0
    for k, f in enumerate(files):
        _, alone = run(extra, [f], d / ("a%d.out" % k))
        got = [r[1:] for r in recs if r[0] == str(k)]
        assert got == [r[1:] for r in alone], "file %d" % k
        n += len(got)
    assert n >= 10


def test_one_stream_per_file_is_byte_identical_to_no_queue(dumps):
    d, files = dumps
    for extra in ([], ["-m", "1"]):
        assert run(["-n", "8"] + extra, files, d / "n8.out") == run(extra, files, d / "n0.out")
