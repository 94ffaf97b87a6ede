"""What the loop-body generators (gen_attn_r64m.py, gen_attn_r64x.py, gen_attn_h64m.py, gen_attn_h64x.py, gen_gemm_t384.py)
share: register names, the instruction list with its ablation filter, the LDS-DMA helpers of the attention loops, the loop
over a body's variants (product | timing ablations) and the command line.  The kernels - fragment maps, register plans,
schedules - are documented and written in the generators themselves.

A generator's output depends on its own text and on its command line, never on the environment: everything an emission
consults travels in one Options object that main() builds from argv."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LABDIR = os.path.normpath(os.path.join(HERE, "..", "..", "benchmarks", "lab", "csrc"))


def vr(lo, n=1):
    return f"v{lo}" if n == 1 else f"v[{lo}:{lo + n - 1}]"


class Options:
    """abl: the timing ablations of the variant being emitted (lab builds only; their results are garbage); every other
    field: an experiment switch of the command line (SWITCHES), or what a generator adds with replace()"""

    def __init__(self, abl=(), **fields):
        self.__dict__.update(fields, abl=frozenset(abl))

    def replace(self, **fields):
        return Options(**{**vars(self), **fields})


class Stmt:
    """the instructions of one asm statement.  DROPS is the ablation filter as data: ablation name -> prefixes of the
    instructions it removes; a generator with rules of its own extends add() (or DROPS) in a subclass."""
    DROPS = {"read": ("ds_read",), "wait": ("s_waitcnt lgkmcnt",), "bar": ("s_barrier",)}

    def __init__(self, opt):
        self.opt, self.abl, self.lines = opt, opt.abl, []

    def add(self, s):
        if not any(s.startswith(p) for a in self.abl for p in self.DROPS.get(a, ())):
            self.lines.append(s)

    def label(self, name):
        self.lines.append(name + ":")

    def text(self):
        return "\n".join(f'      "{ln}\\n\\t"' for ln in self.lines)


def lds_dma(s_kg, s_vg, s_tc, s_tmp, kbytes, vbytes, kpiece=0, vpiece=0):
    """-> (dma_m0, dma, advance) of an attention loop whose K / V^T streams have their global source pairs in s[s_kg:+1] /
    s[s_vg:+1] and ring slots of kbytes / vbytes in LDS.  A wave loads either several pieces per tile and stream (piece i of
    kpiece / vpiece bytes, source offset operand %[koff<i>]) or one (i = None, %[koff]).  The "dma" ablation drops all three."""
    def dma_m0(s, which, slot, i=None):
        """the LDS destination of a piece (an MFMA must separate this M0 write from the load that uses it)"""
        if "dma" not in s.abl:
            size, piece = (kbytes, kpiece) if which == "k" else (vbytes, vpiece)
            s.add(f"s_add_i32 m0, %[{which}dst], {slot * size + (i or 0) * piece}")

    def dma(s, which, i=""):
        if "dma" not in s.abl:
            sg = s_kg if which == "k" else s_vg
            s.add(f"global_load_lds_dwordx4 %[{which}off{i}], s[{sg}:{sg + 1}]")

    def advance(s, which):
        """source pair += one tile, unless the stream has reached its last tile (which is then re-loaded)"""
        if "dma" not in s.abl:
            sg = s_kg if which == "k" else s_vg
            s.add(f"s_cmp_lt_i32 s{s_tc}, %[{which}lim]")
            s.add(f"s_cselect_b32 s{s_tmp}, %[{which}step], 0")
            s.add(f"s_add_u32 s{sg}, s{sg}, s{s_tmp}")
            s.add(f"s_addc_u32 s{sg + 1}, s{sg + 1}, 0")

    return dma_m0, dma, advance


def each_variant(opt, variants, out, lab):
    """variants: [(name, ablations)] -> (options, line sink, function-name suffix) of each: the product body ("") goes to the
    list `out`, every named ablation to the list `lab`"""
    for name, abl in variants:
        yield opt.replace(abl=frozenset(abl)), (lab if name else out).append, ("_" + name if name else "")


def _ints(s):
    return tuple(int(x) for x in s.split(","))


def _pairs(s):
    return frozenset(tuple(int(v) for v in it.split(".")) for it in s.split(","))


# the experiment switches: flag -> (parser of its value or None for an on/off flag, default).  Not product options: the
# committed bodies are the defaults', and a run with a switch can neither --check nor write beside them.
SWITCHES = {"pieces": (_ints, "1,3,5,7,9"), "x-pieces": (_pairs, "2.1,2.5,3.1,3.5,4.1"), "x-bar": (int, "2"),
            "l-spread": None, "sum-by-dot2": None, "pk-args": None, "wait-every-step": None}


def main(bodies, switches=()):
    """the command line of a generator.  bodies: [(stem, emit)], emit(opt) -> (product text, ablations text), written
    to <stem>_body.inc here and <stem>_abl.inc in the lab's csrc (or both under --out-dir); switches: the names in SWITCHES
    that this generator knows - any other flag is an error."""
    ap = argparse.ArgumentParser(allow_abbrev=False)
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--check", action="store_true", help="exit 1 unless the committed product bodies are what this script writes")
    mode.add_argument("--lab", action="store_true", help="write the timing ablations instead of the product bodies")
    ap.add_argument("--out-dir", help="write here instead of into the source tree")
    for name in switches:
        kind = SWITCHES[name]
        ap.add_argument("--" + name, **({"action": "store_true"} if kind is None else {"metavar": kind[1]}))
    args = vars(ap.parse_args())
    check, lab, out_dir = args.pop("check"), args.pop("lab"), args.pop("out_dir")
    if any(args.values()):
        if check:
            ap.error("an experiment switch cannot be combined with --check: the committed bodies are the defaults'")
        if not out_dir or os.path.realpath(out_dir) in (os.path.realpath(HERE), os.path.realpath(LABDIR)):
            ap.error("an experiment switch needs --out-dir DIR outside the source tree's generated files")
    for name in switches:
        if SWITCHES[name] is not None:
            args[name.replace("-", "_")] = SWITCHES[name][0](args[name.replace("-", "_")] or SWITCHES[name][1])
    ok = True
    for stem, emit in bodies:
        text = emit(Options(**args))[1 if lab else 0]
        path = os.path.join(out_dir or (LABDIR if lab else HERE), stem + ("_abl.inc" if lab else "_body.inc"))
        same = os.path.exists(path) and open(path).read() == text
        if check:
            ok = ok and same
            continue
        if not same:                                      # identical content keeps its mtime (make)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            open(path, "w").write(text)
        print(f"wrote {path}: {text.count(chr(10))} lines")
    sys.exit(0 if ok else 1)
