"""The host-side launch rules of libaqua_hip.so restated in plain Python: given an entry point, an action kind, a restart
mode, a shared or per-world obstacle table, its row count K and the batch size N, which kernel instantiations does the
call launch?

The rules are those of aqua_hip.hip -- launch_step / launch_step_ns / launch_step_ns_range (one launch per step, shared
table), aqua_rollout_fused_f32 (the fused rollout), launch_step_tables and aqua_rollout_tables_fused_f32 (per-world
tables).  Every threshold they use is read from the sources' constexpr / #define lines (THRESHOLDS), never copied, so
that a retuned threshold moves the test cells built on it along with it.

Names are in the form llvm-readelf --demangle prints them, with the namespace and the parameter list taken off
(canonical()): "step_ns_kernel<2, true, false, false>", "rollout_tables16_kernel<1, 2>", "tick_kernel".
tests/test_kernel_coverage.py checks this model against the built code object; tests/test_dispatch_matrix.py runs its
cells on the GPU against the oracle.
"""
import ast
import operator
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "include", "aqua_hip.h"),
           os.path.join(ROOT, "aquaticgymenv_amd", "csrc", "aqua_device.hpp"),
           os.path.join(ROOT, "aquaticgymenv_amd", "csrc", "aqua_hip.hip")]

# ------------------------------------------------------------------------------------------------ thresholds
_BINOPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.FloorDiv: operator.floordiv,
           ast.LShift: operator.lshift, ast.RShift: operator.rshift, ast.BitOr: operator.or_, ast.BitAnd: operator.and_}


def _eval(expr, names):
    """an integer constant expression of the C++ sources (literals, casts like int64_t(1), + - * / << >> | &, names
    defined earlier); None if it is anything else"""
    expr = re.sub(r"\b(?:u?int(?:8|16|32|64)_t|size_t|unsigned|int)\s*\(", "(", expr)      # int64_t(1) -> (1)
    expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)(?:[uU]?[lL]{0,2}|[lL]{1,2}[uU]?)\b", r"\1", expr)   # 1u, 1ull -> 1
    expr = expr.replace("/", "//").replace("true", "1").replace("false", "0")
    try:
        tree = ast.parse(expr.strip(), mode="eval")
    except SyntaxError:
        return None

    def ev(node):
        if isinstance(node, ast.Expression):
            return ev(node.body)
        if isinstance(node, ast.Constant) and isinstance(node.value, int):
            return node.value
        if isinstance(node, ast.Name) and node.id in names:
            return names[node.id]
        if isinstance(node, ast.BinOp) and type(node.op) in _BINOPS:
            return _BINOPS[type(node.op)](ev(node.left), ev(node.right))
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            return -ev(node.operand)
        raise ValueError(ast.dump(node))

    try:
        return ev(tree)
    except (ValueError, KeyError):
        return None


def _split_top(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "([{"
        depth -= ch in ")]}"
        if ch == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += ch
    return out + [cur]


_FLOAT = re.compile(r"\s*([-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?)[fF]?\s*$")


def read_thresholds(paths=SOURCES, floats=False):
    """every integer `#define NAME value` and namespace-level `constexpr <type> NAME = value[, NAME = value];` of the
    sources, in order (later definitions may use earlier ones); with `floats`, also the `constexpr float|double` ones
    whose value is a plain literal (1.0e-4f -> 1e-4, the literal's value in double, not rounded to float)"""
    names = {}
    for path in paths:
        with open(path) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        for line in text.splitlines():
            line = line.split("//")[0]
            m = re.match(r"\s*#define\s+([A-Z_][A-Z0-9_]*)\s+(\S.*)$", line)
            if m:
                v = _eval(m.group(2), names)
                if v is not None:
                    names[m.group(1)] = v
                continue
            m = re.match(r"\s*(?:static\s+)?constexpr\s+([\w:]+)\s+(.*?);", line)
            if m:
                real = m.group(1) in ("float", "double")
                for decl in _split_top(m.group(2)):
                    d = re.match(r"\s*([A-Za-z_]\w*)\s*=\s*(.+)$", decl)
                    f = _FLOAT.match(d.group(2)) if d and real and floats else None
                    if f:
                        names.setdefault(d.group(1), float(f.group(1)))
                    elif d:
                        v = _eval(d.group(2), names)
                        if v is not None:
                            names.setdefault(d.group(1), v)
    return names


THRESHOLDS = read_thresholds()
C = THRESHOLDS

KINDS = {"u8": C["AQUA_ACT_U8"], "i32": C["AQUA_ACT_I32"], "i64": C["AQUA_ACT_I64"], "f32x2": C["AQUA_ACT_F32X2"],
         "sample_d": C["AQUA_ACT_SAMPLE_D"], "sample_c": C["AQUA_ACT_SAMPLE_C"], "bearing": C["AQUA_ACT_BEARING"]}
STORED = ("u8", "i32", "i64", "f32x2")
CONTINUOUS = ("f32x2", "sample_c")
MODES = (C["AQUA_RESET_NONE"], C["AQUA_RESET_SAME_STEP"], C["AQUA_RESET_NEXT_STEP"])

# entry points of BatchedAqua (aquaticgymenv_amd/batched.py)
SHARED_ENTRIES = ("step", "rollout", "fused", "graph", "graph_fused", "graph_step")
TABLE_ENTRIES = ("step", "rollout", "fused", "graph", "graph_fused")


def _b(v):
    return "true" if v else "false"


def canonical(demangled):
    """'void (anonymous namespace)::step_kernel<0, true, false, false>((anonymous namespace)::NsArgs) (.kd)'
    -> 'step_kernel<0, true, false, false>'"""
    s = demangled.strip()
    if s.endswith("(.kd)"):
        s = s[:-5].strip()
    s = s.replace("(anonymous namespace)::", "")
    if s.startswith("void "):
        s = s[5:]
    m = re.match(r"[A-Za-z_]\w*", s)
    if not m:
        return s
    end = m.end()
    if end < len(s) and s[end] == "<":
        depth = 0
        for j in range(end, len(s)):
            depth += s[j] == "<"
            depth -= s[j] == ">"
            if depth == 0:
                end = j + 1
                break
    return s[:end]


# ------------------------------------------------------------------------------------------------ launch rules
def step_kernels(kind, mode, K, N):
    """one step of a batch with one obstacle table: launch_step (modes 0, 1) or launch_step_ns (mode 2)"""
    ak = KINDS[kind]
    small = C["NS_TABLE_ROWS"] > 0 and K <= C["NS_TABLE_ROWS"]
    if mode == C["AQUA_RESET_NEXT_STEP"]:
        interleave = N >= C["NS_INTERLEAVE_MIN"]
        wb = C["STORE_WB_NEXT_STEP_MIN"] <= N <= C["STORE_WB_NEXT_STEP_MAX"]
        return {"step_ns_kernel<%d, %s, %s, %s>" % (ak, _b(small), _b(interleave or wb), _b(wb))}
    plain = mode == C["AQUA_RESET_NONE"]
    wb = not plain and N >= C["STORE_WB_SAME_STEP_MIN"]
    return {"step_kernel<%d, %s, %s, %s>" % (ak, _b(small), _b(not plain), _b(wb))}


def fused_kernels(kind, mode, K):
    """aqua_rollout_fused_f32: the quick table for 0 < K <= QUICK_MAX (K == 0 is NOT small here, unlike in step())"""
    small = 0 < K <= C["QUICK_MAX"]
    return {"rollout_kernel<%d, %s, %d>" % (KINDS[kind], _b(small), mode)}


def step_tables_kernels(kind, mode, K, N):
    """launch_step_tables (one launch per step, per-world tables)"""
    ak = KINDS[kind]
    kreg, wide_max, wide_min = C["TABLES_KREG"], C["TABLES_KREG_WIDE"], C["TABLES_KREG_WIDE_MIN"]
    short, long_, long_min = C["SINK_SPLIT_SHORT"], C["SINK_SPLIT_LONG"], C["SINK_SPLIT_LONG_MIN_ROWS"]
    ns_mode = C["TABLES_NEXT_STEP_TILE"]
    wide = wide_min <= K <= wide_max and mode != 0
    regs = K <= kreg or wide
    if mode == C["AQUA_RESET_NEXT_STEP"]:
        # rows in registers: restart inside the tile; otherwise the rows are handed over as they are streamed (ns_sink).
        # step_tables_ns_kernel (the launch split by role) is reached only with -DAQUA_TABLES_ROLE_SPLIT.
        if regs:
            return {"step_tables_kernel<%d, %d, %d, %d>" % (ak, ns_mode, wide_max if wide else kreg, short)}
        return {"step_tables_kernel<%d, %d, 0, %d>" % (ak, ns_mode, long_ if K >= long_min else short)}
    if regs:
        return {"step_tables_kernel<%d, %d, %d, %d>" % (ak, mode, wide_max if wide else kreg, short)}
    if mode:
        split = long_ if K >= long_min else (short if K > wide_max else 1)
        return {"step_tables_kernel<%d, %d, 0, %d>" % (ak, mode, split)}
    return {"step_tables_kernel<%d, 0, 0, %d>" % (ak, short)}


def fused_tables_kernels(kind, mode, K):
    """aqua_rollout_tables_fused_f32: one LDS tile per band of row counts"""
    if K > C["FUSED_TABLE_ROWS_MAX"]:
        raise ValueError("no fused per-world rollout for K=%d" % K)
    if K > 32:
        fam = "rollout_tables64_kernel"
    elif K > 16:
        fam = "rollout_tables32_kernel"
    elif K > C["TABLES_KREG"]:
        fam = "rollout_tables16_kernel"
    else:
        fam = "rollout_tables_kernel"
    return {"%s<%d, %d>" % (fam, KINDS[kind], mode)}


def launched(entry, kind, mode, K, N, per_world=False, T=3, with_reset=True):
    """the set of this library's kernels that BatchedAqua(N, <table>, auto_reset=mode) launches for reset() (with_reset)
    followed by `entry` over T steps:
      step         step() T times                       rollout      rollout(T, fused=False)
      fused        rollout(T, fused=True)                graph        capture_rollout(T) + launch()
      graph_fused  capture_rollout(T, fused=True) + launch()          graph_step   capture_step() + launch()"""
    if kind not in KINDS or mode not in MODES:
        raise ValueError((kind, mode))
    out = set()
    if with_reset:
        out.add("reset_tables_kernel" if per_world else "reset_kernel")
    per_step = (lambda: step_tables_kernels(kind, mode, K, N)) if per_world else (lambda: step_kernels(kind, mode, K, N))
    if entry in ("step", "rollout"):
        out |= per_step()
    elif entry == "fused":
        out |= fused_tables_kernels(kind, mode, K) if per_world else fused_kernels(kind, mode, K)
    elif entry == "graph":
        out |= per_step()
        if T == 1:                      # T >= 2: the first and last step launches advance the tick base themselves
            out.add("tick_kernel")
    elif entry == "graph_fused":
        out |= fused_tables_kernels(kind, mode, K) if per_world else fused_kernels(kind, mode, K)
        out.add("tick_kernel")
    elif entry == "graph_step":
        out |= per_step()
        out.add("tick_kernel")
    else:
        raise ValueError("unknown entry %r" % (entry,))
    return out
