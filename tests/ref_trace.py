"""Readers for what the reference's own programs (oracle/_ref, built from its unmodified sources against
oracle/refshim/binfhecontext.h) leave behind: the stand-in's call trace and the `Processing: X of Y` progress lines of
Circuit::Clock.  Test infrastructure; nothing of the product is imported here.

The trace (format: oracle/refshim/binfhecontext.h) is matched to a netlist STRUCTURALLY, never by id order: every
ciphertext id gets a canonical form built bottom-up from its record -- the k-th Encrypt of a SetInput is ("E", k),
EvalNOT(x) is ("N", form(x)), EvalBinGate(op, x, y) is (op, form(x), form(y)) -- and the netlist says which forms a run
must contain: a LOAD is ("E", position in file order), NOT / AND / OR are one record, and an XOR is the five records of
src/gate.cpp:198-202, OR(AND(a, NOT b), AND(NOT a, b)), in that operand order.  Ids of equal form are the same
function of the same inputs (and, gate evaluation being deterministic, the same ciphertext), so the match is a multiset
equality: every gate finds its records and every record is used.
"""
import os
import re
import subprocess
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = os.environ.get("BCE_REFERENCE", "/root/reference")
TB_NAMES = ["TB_adder_2bit", "TB_adders", "TB_aes", "TB_comparators", "TB_md5", "TB_multipliers", "TB_parity", "TB_sha256"]
REF_PROGRAMS = ["ref_run_bits", "ref_run_oracle", "ref_assemble"] + TB_NAMES


def have_binaries():
    return all(os.path.exists(os.path.join(REF_BIN, p)) for p in REF_PROGRAMS)


def have_checkout():
    return os.path.exists(os.path.join(REF_SRC, "src", "circuit.cpp"))


class Run:
    """One SetInput + Clock of the trace."""

    def __init__(self):
        self.enc = []        # (id, bit) of the Encrypt calls of SetInput, in call order
        self.fix_enc = []    # (id, bit) of Encrypt calls made inside gate tasks (verify mode's repairs)
        self.nots = []       # (out, in)
        self.gates = []      # (op, out, in0, in1)
        self.out_dec = []    # (id, bit) of the Decrypt calls of the OUTPUT gates (serial part of _ExecuteGates)
        self.task_dec = 0    # Decrypt calls inside gate tasks (src/gate.cpp:72-77 and the verify checks)
        self.rows = {}       # id -> uint64 row (oracle back end)


def read_trace(path):
    """-> list of Run.  A run starts at the first SetInput-level Encrypt after anything that is not one."""
    runs, cur, in_input = [], None, False
    for line in open(path):
        t = line.split()
        if not t:
            continue
        k = t[0]
        if k == "M":
            in_input = False
            continue
        if k == "C":
            cur.rows[int(t[1])] = np.array(t[2:], dtype=np.uint64)
            continue
        if k == "E" and int(t[3]) == 0:
            if not in_input:
                cur = Run()
                runs.append(cur)
                in_input = True
            cur.enc.append((int(t[1]), int(t[2])))
            continue
        in_input = False
        if k == "E":
            cur.fix_enc.append((int(t[1]), int(t[2])))
        elif k == "N":
            cur.nots.append((int(t[1]), int(t[2])))
        elif k == "G":
            cur.gates.append((t[1], int(t[2]), int(t[3]), int(t[4])))
        elif k == "D":
            if int(t[3]) == 0:
                cur.out_dec.append((int(t[1]), int(t[2])))
            else:
                cur.task_dec += 1
        else:
            raise ValueError("unreadable trace record: " + line)
    return runs


class Forms:
    """interns canonical forms as small integers"""

    def __init__(self):
        self.ids = {}
        self.keys = []
        self.norm = {}

    def __call__(self, *key):
        v = self.ids.get(key)
        if v is None:
            v = self.ids[key] = len(self.ids)
            self.keys.append(key)
        return v

    def normal(self, f):
        """the form with every EvalNOT(EvalNOT(x)) replaced by x: negating an LWE ciphertext twice, (-a, q/4 - b) of
        (-a, q/4 - b), gives back the very same words, so forms of one normal form are still one ciphertext"""
        todo = [f]
        while todo:                                  # iterative: the forms of a deep circuit nest deeply
            g = todo[-1]
            if g in self.norm:
                todo.pop()
                continue
            key = self.keys[g]
            if key[0] == "E":
                self.norm[g] = g
                todo.pop()
                continue
            kids = [k for k in key[1:] if k not in self.norm]
            if kids:
                todo.extend(kids)
                continue
            args = [self.norm[k] for k in key[1:]]
            if key[0] == "N" and self.keys[args[0]][0] == "N":
                self.norm[g] = self.keys[args[0]][1]
            else:
                self.norm[g] = self(key[0], *args)
                self.norm.setdefault(self.norm[g], self.norm[g])
            todo.pop()
        return self.norm[f]


class MatchError(AssertionError):
    pass


def gate_text(g):
    op, dst, a, b = g
    return "R%d = %s(R%d)" % (dst, op, a) if op == "NOT" else "R%d = %s(R%d, R%d)" % (dst, op, a, b)


def match(nl, run, forms_out=None):
    """Match one run to netlist `nl` (oracle_walk.Netlist).  Returns {register: [ids of its form]}; raises MatchError
    naming the first gate without its records, or the first record no gate accounts for.  A dict passed as `forms_out`
    receives the interner ("F") and every register's form ("reg_form"), for plan_forms below."""
    F = Forms()
    if len(run.enc) != len(nl.loads):
        raise MatchError("SetInput made %d Encrypt calls for %d LOADs" % (len(run.enc), len(nl.loads)))
    if run.fix_enc:
        raise MatchError("%d Encrypt calls inside gate tasks (verify-mode repairs)" % len(run.fix_enc))
    form_of = {}                                   # trace id -> form
    for k, (i, _) in enumerate(run.enc):
        form_of[i] = F("E", k)
    have = Counter()
    rec_text = {}
    pending = [("N", o, a, -1) for o, a in run.nots] + list(run.gates)
    pending.sort(key=lambda r: r[1])               # an id is handed out after its inputs': ascending id is topological
    for op, o, a, b in pending:
        if a not in form_of or (b >= 0 and b not in form_of):
            raise MatchError("trace record %s %d %d %d uses an id nothing produced" % (op, o, a, b))
        f = F(op, form_of[a]) if op == "N" else F(op, form_of[a], form_of[b])
        form_of[o] = f
        have[f] += 1
        rec_text[f] = "%s %d <- %d %d" % (op, o, a, b)
    want = Counter()
    reg_form = {}
    for k, (reg, _, _) in enumerate(nl.loads):
        reg_form[reg] = F("E", k)

    def need(f, g):
        want[f] += 1
        if want[f] > have[f]:
            raise MatchError("gate %s: no trace record for it (the trace evaluates something else there)" % gate_text(g))
        return f

    for g in nl.gates:
        op, dst, a, b = g
        if op == "NOT":
            reg_form[dst] = need(F("N", reg_form[a]), g)
        elif op in ("AND", "OR"):
            reg_form[dst] = need(F(op, reg_form[a], reg_form[b]), g)
        elif op == "XOR":                          # src/gate.cpp:198-202
            fa, fb = reg_form[a], reg_form[b]
            na = need(F("N", fa), g)
            nb = need(F("N", fb), g)
            t1 = need(F("AND", fa, nb), g)
            t2 = need(F("AND", na, fb), g)
            reg_form[dst] = need(F("OR", t1, t2), g)
        else:
            raise MatchError("unknown netlist op " + op)
    for f, n in have.items():
        if want[f] != n:
            raise MatchError("trace record %s (x%d) is used by no gate of the netlist (x%d)" % (rec_text[f], n, want[f]))
    if forms_out is not None:
        forms_out.update(F=F, reg_form=reg_form)
    by_form = {}
    for i, f in form_of.items():
        by_form.setdefault(f, []).append(i)
    return {reg: sorted(by_form[f]) for reg, f in reg_form.items()}


_DESC_OPS = {0: "OR", 1: "AND", 2: "NOR", 3: "NAND", 4: "XOR_FAST", 5: "XNOR_FAST"}


def plan_forms(F, nl, steps):
    """Forms of the slots a descriptor schedule of OURS writes (Circuit.relevel_plan(): lists of (op, in0, in1, out, neg0,
    neg1), a negation flag = EvalNOT of that operand), in the interner of a matched reference run: slot -> form."""
    form = {reg: F("E", k) for k, (reg, _, _) in enumerate(nl.loads)}
    for step in steps:
        done = {}
        for op, a, b, out, n0, n1 in step:              # the descriptors of a step read the pool as it was before the step
            fa = F("N", form[a]) if n0 else form[a]
            if op == 16:
                done[out] = F("N", form[a])
            elif op == 18:
                done[out] = form[a]
            else:
                fb = F("N", form[b]) if n1 else form[b]
                done[out] = F(_DESC_OPS[op], fa, fb)
        form.update(done)
    return form


def input_bits(nl, run):
    """the bits SetInput encrypted, as buses: [[bit 0, bit 1, ...] of In1, ... of In2]"""
    n_bus = 1 + max(v for _, v, _ in nl.loads)
    buses = [dict() for _ in range(n_bus)]
    for (reg, value, bit), (_, b) in zip(nl.loads, run.enc):
        buses[value][bit] = b
    return [[bus[k] for k in range(len(bus))] for bus in buses]


def output_bits(nl, run, reg_ids):
    """the bits the OUTPUT gates decrypted, by output bit"""
    dec = dict(run.out_dec)
    if len(run.out_dec) != len(nl.stores):
        raise MatchError("%d OUTPUT decrypts for %d STOREs" % (len(run.out_dec), len(nl.stores)))
    out = []
    for k in range(1 + max(nl.stores)):
        hit = [dec[i] for i in reg_ids[nl.stores[k]] if i in dec]
        if not hit:
            raise MatchError("Out%d = STORE(R%d): its ciphertext was never decrypted as an output" % (k, nl.stores[k]))
        out.append(hit[0])
    return out


def register_rows(run, reg_ids):
    """register -> its row (oracle back end); ids of one form must carry one ciphertext"""
    rows = {}
    for reg, ids in reg_ids.items():
        r = run.rows[ids[0]]
        for i in ids[1:]:
            assert np.array_equal(run.rows[i], r), "ids %d and %d: same function of the same inputs, different rows" % (ids[0], i)
        rows[reg] = r
    return rows


_PROC = re.compile(r"Processing: (\d+) of (\d+)")


def clock_rounds(stdout):
    """stdout of a reference program -> per Clock(), the gates done per round (OUTPUT gates included):
    Circuit::_ExecuteGates prints the running `Processing: X of Y` once per round; a Clock ends at `### Total time`."""
    clocks, cur, last = [], [], 0
    for piece in re.split(r"[\r\n]+", stdout):
        m = _PROC.search(piece)
        if m:
            x = int(m.group(1))
            cur.append(x - last)
            last = x
        if "### Total time" in piece:
            clocks.append(cur)
            cur, last = [], 0
    return clocks


def expected_rounds(nl, ready):
    """`ready` = the gate rounds of a walker (oracle_walk.rounds shape: lists of (op, dst, a, b)) -> gates per round as
    the reference counts them: an OUTPUT gate runs in the round after its register was produced (round 0 for a LOAD)."""
    level = {r: -1 for r, _, _ in nl.loads}
    for lv, gates in enumerate(ready):
        for g in gates:
            level[g[1]] = lv
    counts = [len(g) for g in ready]
    for reg in nl.stores.values():
        lv = level[reg] + 1
        while len(counts) <= lv:
            counts.append(0)
        counts[lv] += 1
    return counts


def run_program(name, args, cwd=None, trace=None, seed=None, timeout=600):
    """Run oracle/_ref/<name>; returns stdout.  `trace` names the trace file (removed first), `seed` the oracle seed."""
    env = dict(os.environ)
    env.pop("BCE_REF_TRACE", None)
    env.pop("BCE_REF_ENC_BASE", None)
    if trace is not None:
        if os.path.exists(trace):
            os.remove(trace)
        env["BCE_REF_TRACE"] = trace
    if seed is not None:
        env["BCE_REF_SEED"] = str(int(seed))
    p = subprocess.run([os.path.join(REF_BIN, name)] + [str(a) for a in args], cwd=cwd, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)
    assert p.returncode == 0, "%s %s failed (%d):\n%s\n%s" % (name, args, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "fixing" not in p.stderr and "error" not in p.stderr.lower(), p.stderr[-2000:]
    return p.stdout


def vector_arg(buses):
    """input buses -> ref_run's vector argument (bit 0 first, buses joined by ',')"""
    return ",".join("".join(str(int(b)) for b in bus) for bus in buses)
