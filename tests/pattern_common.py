"""Shared by tests/test_contact_patterns_host.py and tests/test_contact_patterns_gpu.py: whole-body schedules that put every one of the 16
contact patterns, and touchdown sets of every size, in front of the pattern-dependent kernel code (wb_select's row compaction, the m <= 6 branch
of wb_kkt_column, the LQ knot's per-foot slot lookups, the lane quad's rank `before` / block `cb`, the never-stored structural zeros of the
contact-solve cache, the friction-pyramid constraint index, the impact over next_contact & ~contact).

Families, p one of P16 (itertools.product order), rot(p) = p[1:] + p[:1]:

  into_stance(p)    schedule (p, 1111),         horizons (3, 2),    last_next 1111   phase 0 runs on p and ends with the touchdown of ~p (0 - 4 feet)
  out_of_stance(p)  schedule (1111, p),         horizons (3, 2),    last_next p      a lift-off without impact; the last phase runs on p, no successor
  rotate(p)         schedule (1111, p, rot(p)), horizons (2, 3, 2), last_next 1111   lift-off and touchdown at one boundary with asymmetric sets; a
                                                                                     foot that lands in phase 1 is a contact foot of phase 2 under
                                                                                     another rank

States: problems.wb_ensemble_x0(5, 20241222).  Five problems of 7 - 8 knots: the lane-quad wave of 16 knots is partly filled and holds quads of
several problems."""
import itertools

from conftest import pkg

P16 = tuple(itertools.product((0, 1), repeat=4))
STANCE = (1, 1, 1, 1)
SEED = 20241222
BATCH = 5
FAMILIES = ("into_stance", "out_of_stance", "rotate")
RECONFIGURE_ORDER = ((1, 1, 1, 1), (0, 1, 1, 1), (0, 0, 0, 1), (1, 0, 1, 0), (1, 0, 0, 0), (1, 1, 1, 0))      # shrinks and grows the contact set
SIM_PATTERNS = ((0, 1, 1, 1), (0, 0, 0, 1), (1, 0, 1, 0))


def rot(p):
    return tuple(p[1:]) + tuple(p[:1])


def name(p):
    return "".join(str(c) for c in p)


def into_stance(p):
    return dict(schedule=(tuple(p), STANCE), horizons=(3, 2), last_next=STANCE)


def out_of_stance(p):
    return dict(schedule=(STANCE, tuple(p)), horizons=(3, 2), last_next=tuple(p))


def rotate(p):
    return dict(schedule=(STANCE, tuple(p), rot(p)), horizons=(2, 3, 2), last_next=STANCE)


def case(family, p):
    """Phase descriptors of one case."""
    return pkg.problems.wb_trot_problem(**{"into_stance": into_stance, "out_of_stance": out_of_stance, "rotate": rotate}[family](p))


def states(batch=BATCH):
    return pkg.problems.wb_ensemble_x0(batch, SEED)


def solve_options():
    """The short full solves: 2 AL x 3 DDP iterations."""
    return pkg.mhpc_ddp_setting(max_AL_iter=2, max_DDP_iter=3)


def worst_ratio(report):
    """Largest error / tolerance of a parity_common.run_steps report (keys (step, field, phase)) or compare_solve report (keys (field, phase)),
    per field group: rollout, lq, sweep (without K), K, linear - or solve, K."""
    out = {}
    for key, (err, sc, own, tol) in report.items():
        g = "K" if key[-2] == "K" else (key[0].rstrip("0123456789") if len(key) == 3 else "solve")
        out[g] = max(out.get(g, 0.0), err / tol)
    return out
