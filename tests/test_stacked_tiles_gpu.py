"""Device stage of the stacked-GRU tile tests: EVERY row of the case table of tests/stacked_cases.py on the MI355X, against the float64
references of tests/width_ref.py.  python -m pytest tests -m gpu

What the emulator stage (tests/test_stacked_tiles_cpu.py) cannot see is the hand-off of the resident kernel as it really is --
write-through publishes of the limb images, per-octet flags, several tile sets polling at once, blocks of eight layers waiting on each
other -- the KPW = 16 instance of H = 1024 with its operand ring at three and four tiles per block, the any-H kernel's 256 resident
blocks behind the grid barrier at three layers, and the 512-block launches of H = 2048.

Every buffer is a view of exactly the size the library asks for inside one NaN-filled device allocation (width_util's header): a
pass that reads or writes past a buffer fails the comparison or the guard check, it cannot fault.  A hand-off that never arrives ends
after 2^22 polls with status word 3, which the drivers assert to be zero.

Bounds: the device bounds the project already uses, unchanged -- TIGHT_PASS = 5e-6 per pass against the reference, TIGHT_KERNELS = 3e-6
between the resident and the any-H kernel (tests/stacked_util.py).  Every measured distance is printed (run with -s) and, when
CYCLEVAE_REPORT_DIR names a directory, appended to stacked_tiles_gpu_report.txt; profiles/stacked_tiles_notes.md keeps them."""
import pytest

import stacked_cases as sc
import width_util as wu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

note = wu.make_note("stacked_tiles_gpu_report.txt")
ids = lambda cases: [c.id for c in cases]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    """A context of its own on the loaded library: the max_rt set here never reaches the passes of other tests."""
    import gru_vae
    ctx = gru_vae._lib().new_context()
    yield ctx
    torch.cuda.synchronize()
    ctx.close()


@pytest.fixture(scope="module")
def mem(lib, dev):
    return wu.TorchMem(lib, dev)


@pytest.fixture(scope="module")
def refs():
    return sc.make_refs()


@pytest.mark.parametrize("c", sc.STACK_CASES, ids=ids(sc.STACK_CASES))
def test_stacked_pass_at_tiling(mem, refs, options, c):
    """The row's plan {path, Bp, rts, tiles}, then: whole pass, two windows with the carried (y_last, h [L,B,H]), h_in with an
    off-manifold y_in, T = 1; at the `twin` rows also the per-step launches, bit for bit."""
    sc.run_stack_case(mem, c, refs(c), note, sc.TIGHT_PASS, options)


@pytest.mark.parametrize("rows", sorted(sc.TILINGS))
def test_resident_bits_do_not_depend_on_the_tiling(mem, refs, options, rows):
    """33, 97 and 160 rows under every resident tiling max_rt 0 .. 3 gives: identical bits of trj_out, y_last and h_last."""
    sc.run_tilings(mem, rows, refs(sc.h64_case(rows)), note, sc.TIGHT_PASS, options)


def test_rows_at_tile_edges_are_independent_of_the_batch(mem):
    """Rows 0, 31, 32, 64, 96 of the 97-row batch as a batch of five, and row 96 alone: the bits they have in the full batch."""
    sc.run_row_independence(mem, note)


@pytest.mark.parametrize("c", sc.VERSUS_CASES, ids=ids(sc.VERSUS_CASES))
def test_resident_against_any_h_kernel(mem, options, c):
    sc.run_versus(mem, c, note, sc.TIGHT_KERNELS, options)
