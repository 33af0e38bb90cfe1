"""Pure-Python restatement of the list expressions, shared by test_list_expr_cpu.py and test_gpu_list_expr.py.
Values are Python ints / floats / bools / strs, None is NULL, a list is a Python list."""
import math

T = 2048  # kExplodeTile, the tile of virtual (row, position) slots (csrc/capsmi_impl.h; pinned by test_list_expr_cpu)


def ref_range(start, end, step=1):
    """Scala's start.to(end, step) over Long: inclusive, empty on the wrong side, step 0 an error."""
    if step == 0:
        raise ValueError("range: step 0")
    out, x = [], start
    while (x <= end) if step > 0 else (x >= end):
        out.append(x)
        x += step  # Python ints: no overflow
    return out


def ref_size(lst):
    return None if lst is None else len(lst)


def ref_index(lst, i):
    if lst is None or i is None or i < 0 or i >= len(lst):
        return None
    return lst[i]


def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def ref_equal(a, b):
    """The interpreter's `=` on non-null values: None when the types cannot be compared; Long against Double as
    doubles; NaN equal to NaN."""
    if _is_num(a) and _is_num(b):
        if isinstance(a, int) and isinstance(b, int):
            return a == b
        x, y = float(a), float(b)
        if math.isnan(x) or math.isnan(y):
            return math.isnan(x) and math.isnan(y)
        return x == y
    if type(a) is not type(b):
        return None
    return a == b


def ref_in_list(x, lst, elem_kind=None):
    """x IN lst, three-valued.  elem_kind: the list's element Python type, which decides comparability even for
    an empty list (the column's type is static)."""
    if x is None or lst is None:
        return None
    if elem_kind is not None:
        num = (int, float)
        if not ((type(x) in num and elem_kind in num) or type(x) is elem_kind):
            return None
    hit = False
    for e in lst:
        r = ref_equal(x, e)
        if r is None:
            return None
        hit = hit or r
    return hit
