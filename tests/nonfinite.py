"""Helpers of tests/test_nonfinite.py: the four-part contract for non-finite values (include/stc_hip.h, "Non-finite values") as one checker.

A case is a function ``run(k, d) -> {name: tensor}`` on a kernel set ``k`` and a dict ``d`` of operands; the checker takes three runs of it:

    want    the float64 run of the CPU restatement (pattern semantics: entries absent from a sparse pattern do not take part, a dense operand
            is dense arithmetic) on the POISONED operands; the same run on the clean operands tells what the poison reaches at all
    got     the code under test on the poisoned operands
    clean   the code under test on the un-poisoned operands

    A  no masking     wherever want is non-finite, got is non-finite (NaN against +-Inf is not compared)
    B  containment    outside the poison's reach -- what want marks or changes, plus the kernel's documented spread unit -- got equals clean BIT FOR BIT
    C  finite part    the elements asserted under B meet the parity tolerance of the kernel's own test against want
    D  reductions     the parameter-gradient / reduction outputs of a launch are one unit: with any non-finite element in want they are held to A only;
                      so is every output when an INF sits in a table that every row reads (the split-operand kernels scale a table by its own
                      maximum; a NaN is dropped by that maximum and is held to B and C like any other poison)

and the self-checks of a case: want has a non-finite element and (unless the poison sits in a table or weight that every row reads) a finite one,
and at least half of the per-row outputs' rows are asserted under B.
"""
import torch

POISONS = {'nan': float('nan'), '+inf': float('inf'), '-inf': float('-inf')}
F32_TOL = 1e-5
GRAD_TOL = 2e-5
BF16_TOL = 2.0 ** -7


class ContractFailure(AssertionError):
    def __init__(self, part, msg):
        super().__init__(f'part {part}: {msg}')
        self.part = part


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def poisoned(operands, name, index, value):
    """A copy of the operand dict with one element of one float operand replaced."""
    out = {k: (v.clone() if isinstance(v, torch.Tensor) else ([t.clone() for t in v] if isinstance(v, list) else v)) for k, v in operands.items()}
    t = out[name[0]][name[1]] if isinstance(name, tuple) else out[name]
    assert t.is_floating_point(), 'poison is data: never an index, count or plan array'
    t[index] = value
    return out


def mapped(operands, fn, ints=None):
    """The operand dict with ``fn`` applied to every floating-point tensor (also inside lists) and ``ints`` to the index tensors; everything
    else is handed on as it is."""
    def one(v):
        if isinstance(v, torch.Tensor):
            return fn(v) if v.is_floating_point() else (v if ints is None else ints(v))
        if isinstance(v, list):
            return [one(t) for t in v]
        return v
    return {k: one(v) for k, v in operands.items()}


def _rows(mask):
    return mask.reshape(-1, mask.shape[-1]) if mask.dim() >= 2 else mask.reshape(-1, 1)


def spread_groups(bad, axis, groups):
    """The reach of a kernel that computes the rows of a group together (a 4-row block, a patch): along ``axis`` every member of a group with a
    marked member is marked, element by element of the other axes.  ``groups``: iterable of index lists (rows in no group stay as they are)."""
    n = bad.shape[axis]
    gid = torch.arange(n) + len(groups)                                    # a row in no group: a group of its own
    for i, g in enumerate(groups):
        gid[torch.as_tensor(g, dtype=torch.long)] = i
    moved = bad.movedim(axis, 0)
    flat = moved.reshape(n, -1)
    hits = torch.zeros(n + len(groups), flat.shape[1], dtype=torch.int32).index_add_(0, gid, flat.to(torch.int32))
    return (hits[gid] > 0).reshape(moved.shape).movedim(0, axis)


def blocks_of(n, size=4):
    return [list(range(s, min(s + size, n))) for s in range(0, n, size)]


def check_contract(tag, want, want_clean, got, clean, kinds, tols=None, spread=None, table_poison=False, default_tol=F32_TOL, coverage=True, expect_nonfinite=True,
                   table_site=False, exempt=None, exempt_strict=True):
    """``kinds[name]``: 'rows' (a per-row output: last axis = the row) or 'reduce' (part D).  ``spread(name, touched, touched of every output) -> reach``.
    ``table_poison``: the whole launch is one unit (part D); ``table_site``: the poison sits in a table all rows read (no row count, whatever the unit);
    ``exempt[name]``: mask (or True: all) of outputs documented to keep the CLEAN run's value, bit for bit, where want is non-finite
    (``exempt_strict=False``: only exempt from A -- an Inf gives the node the smallest activation scale, its finite entries carry no meaning).  ``coverage=False``: an operation that is dense in itself (every row reads the poisoned element's row or column): no row count is asked for.
    Raises ContractFailure naming the part; returns (rows asserted under B, rows of the per-row outputs)."""
    tols = tols or {}
    kept_rows = total_rows = 0
    any_bad = any_finite = any_touched = False
    # part D: the parameter-gradient outputs of ONE launch are one unit -- a node whose gradient maximum is non-finite takes the smallest scale, so
    # what it adds to the launch's other sums (a bias gradient beside a NaN weight gradient) is flushed: finite, and not meaningful
    unit_bad = any(kinds[n_] == 'reduce' and w_ is not None and not bool(torch.isfinite(w_.detach().double()).all()) for n_, w_ in want.items())
    def _touched(name):
        w_ = want[name].detach().cpu().double()
        return ~torch.isfinite(w_) | ~(w_ == want_clean[name].detach().cpu().double())
    touched_all = {n_: _touched(n_) for n_, w_ in want.items() if w_ is not None}      # (a spread unit may depend on another output's reach)
    for name, w in want.items():
        if w is None:
            assert got[name] is None and clean[name] is None
            continue
        w, g, c = w.detach().cpu().double(), got[name].detach().cpu(), clean[name].detach().cpu()
        assert w.shape == g.shape == c.shape, (tag, name)
        bad = ~torch.isfinite(w)
        touched = bad | ~(w == want_clean[name].detach().cpu().double())        # the math's reach: a -Inf gate comes out as a finite 0, and is not the clean value
        any_bad, any_finite, any_touched = any_bad or bool(bad.any()), any_finite or bool((~bad).any()), any_touched or bool(touched.any())
        masked = bad & torch.isfinite(g.double())
        if exempt is not None and name in exempt:                           # the documented exception to A: what the shortcut x * 0 := 0 leaves out
            ex = (torch.ones_like(bad) if exempt[name] is True else exempt[name]) & bad
            same = (bits(g) == bits(c)) | ~torch.isfinite(g.double())          # (non-finite, as the general form has it, or untouched: the clean value)
            if exempt_strict and not bool(same[ex].all()):
                raise ContractFailure('A', f'{tag} {name}: an output exempt from A is neither non-finite nor the clean run\'s value')
            masked &= ~ex
        if bool(masked.any()):
            raise ContractFailure('A', f'{tag} {name}: {int(masked.sum())} of {int(bad.sum())} non-finite results came out finite, first at '
                                       f'{tuple(masked.nonzero()[0].tolist())}')
        if table_poison or (kinds[name] == 'reduce' and unit_bad):
            continue                                                            # part D: one unit
        reach = touched if spread is None else spread(name, touched, touched_all)
        assert bool((reach | ~touched).all())
        keep = ~reach
        if kinds[name] == 'rows':
            r = _rows(keep).all(1)
            total_rows, kept_rows = total_rows + r.numel(), kept_rows + int(r.sum())
        differ = (bits(g) != bits(c)) & keep
        if bool(differ.any()):
            raise ContractFailure('B', f'{tag} {name}: {int(differ.sum())} results outside the reach differ from the clean run, first at '
                                       f'{tuple(differ.nonzero()[0].tolist())}')
        if bool(keep.any()):
            ref = w[keep]
            err = float((g.double()[keep] - ref).abs().max() / ref.abs().max().clamp(min=1e-300))
            tol = tols.get(name, default_tol)
            if not err < tol:
                raise ContractFailure('C', f'{tag} {name}: {err:.3e} >= {tol:.1e} on the finite part')
    # (an Inf may legitimately end as a finite number: tanh(Inf) = 1, sigmoid(-Inf) = 0; a NaN may not)
    assert any_bad if expect_nonfinite else any_touched, (tag, 'the poison reaches nothing: not a case')
    if not (table_poison or table_site):
        assert any_finite, (tag, 'everything is non-finite: containment is not exercised')
        assert not coverage or total_rows == 0 or 2 * kept_rows >= total_rows, (tag, f'only {kept_rows} of {total_rows} rows asserted under containment')
    return kept_rows, total_rows
