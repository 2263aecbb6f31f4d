"""The training GEMM wrappers on their own on the device (gemm_nt / gemm_tn / gemm_ks / colsum_launch behind cvae_selftest_gemm): the
case table of tests/gemm_util.py -- every LDS tile x contraction split x edge class, the simple kernels, the mask epilogue -- against
the float64 numpy reference, bit for bit (integer operands, exact in any summation order), and one N(0, 1) shape per kernel and
tile against the derived bound |d| <= 2 (depth + slices + 2) 2^-24 (sum |a||b| + |bias| + |C_old|).  python -m pytest tests -m gpu

The same table has run through the sanitizer driver and the emulator first (tests/test_emu_gemm.py); the library refuses a case
outside a kernel's operand contract.  Operands are views inside ONE larger NaN-filled device allocation: a read outside a contract
lands in allocated memory and gives NaN (a failure), a write outside a view is seen in the guard floats.  The largest |d| / bound of
the real-valued run is printed (run with -s) and, when CYCLEVAE_REPORT_DIR names a directory, appended to gemm_gpu_report.txt."""
import os

import numpy as np
import pytest

import gemm_util as gu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPORT_DIR = os.environ.get("CYCLEVAE_REPORT_DIR")


def note(msg):
    if REPORT_DIR:
        os.makedirs(REPORT_DIR, exist_ok=True)
        with open(os.path.join(REPORT_DIR, "gemm_gpu_report.txt"), "a") as f:
            f.write(msg + "\n")
    print(msg)


class TorchArena(gu.NumpyArena):
    """gemm_util.NumpyArena over one device tensor."""

    def __init__(self, dev, floats=1 << 20):
        self.buf = torch.full((floats,), float("nan"), dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.reset()

    def write(self, off, a):
        self.buf[off:off + a.size].copy_(torch.from_numpy(np.ascontiguousarray(a)))

    def read(self, off, n):
        return self.buf[off:off + n].cpu().numpy()

    def address(self, off):
        return self.buf.data_ptr() + 4 * off

    def sync(self):
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def lib():
    """A context of its own on the loaded library: the options set here never reach the passes of other tests."""
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import gru_vae
    ctx = gru_vae._lib().new_context()
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.fixture(scope="module")
def bench(lib):
    dev = torch.device("cuda:0")
    nbytes = lib.selftest_gemm_work_bytes()
    work = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)           # allocated and zeroed once
    assert work.data_ptr() % 16 == 0
    return {"arena": TorchArena(dev, 6 << 20), "work": work, "addr": work.data_ptr(), "bytes": nbytes,
            "counters": lambda: work[-gu.CNT:].cpu().numpy(), "stream": torch.cuda.current_stream().cuda_stream}


def run_all(lib, options, bench, cases, real=False):
    worst = 0.0
    for c in cases:
        options(**c.options())
        worst = max(worst, gu.run_case(lib, bench["arena"], c, bench["addr"], bench["bytes"], bench["counters"], real=real,
                                       stream=bench["stream"]))
    return worst


@pytest.mark.parametrize("kind", [gu.NT, gu.TN, gu.KS, gu.COLSUM], ids=["nt", "tn", "ks", "colsum"])
def test_integer_table_bit_for_bit(lib, options, bench, kind):
    run_all(lib, options, bench, [c for c in gu.table() if c.kind == kind])


def test_real_valued_within_derived_bound(lib, options, bench):
    worst = run_all(lib, options, bench, gu.table(real=True), real=True)
    note("training GEMMs, N(0,1) operands, %d cases: largest |d| / bound = %.3f" % (len(gu.table(real=True)), worst))
    assert worst <= 1.0


def test_split_dropped_when_padded_tiles_overflow_the_work_space(lib, options, bench):
    """gemm_nt / gemm_tn keep a forced split only when the PADDED tiles fit the work space: 16 slices of a 1025 x 993 output fit as
    floats (16.3 M <= 2^24) but not as 33 x 32 tiles of 32 x 32 (17.3 M), and a 2049 x 2048 output has 65 x 64 = 4160 > 4096 tiles
    (one arrival counter each).  The wrapper must then run ONE slice and report it -- an output this large is too slow for the
    emulator stages, so these three cases run here only; the kernels are the unsplit 32 x 32 ones the table covers."""
    cases = [gu.nt_case(1025, 993, 272, form=0, bias=1, force=10116), gu.nt_case(2049, 2048, 32, form=0, acc=1, force=10102),
             gu.tn_case(32, 2049, 2048, form=0, force=10102)]
    assert [c.e_nz for c in cases] == [1, 1, 1] and all(c.split for c in cases)
    run_all(lib, options, bench, cases)
