"""Pure-Python restatement of the two modes of capsmi_with_mask_list_column, shared by test_entity_functions_cpu.py
and test_gpu_entity_functions.py.  A column is a list of (value, valid) pairs, one per row; the result is one Python
list of names per row, never None (CAPSFunctions.scala:73-91 as read: filterWithMask's `case (label, true)` and
filterNotNull's `value != null` skip null elements, so a row of nulls gives [])."""

MASK_TRUE, MASK_NOT_NULL = 0, 1  # include/capsmi.h CAPSMI_MASK_*


def ref_mask_list(mode, columns, names):
    """columns: per column a list of (value, valid) over the rows; names: per column its name, in the caller's
    order (which is kept)."""
    assert len(columns) == len(names)
    n = len(columns[0]) if columns else 0
    out = []
    for r in range(n):
        row = []
        for col, name in zip(columns, names):
            value, valid = col[r]
            if valid and (mode == MASK_NOT_NULL or bool(value)):
                row.append(name)
        out.append(row)
    return out


def ref_labels(columns, names):
    """labels(): the names sorted (SparkSQLExprMapper.scala:198), the flags non-null and TRUE."""
    order = sorted(range(len(names)), key=lambda i: names[i])
    return ref_mask_list(MASK_TRUE, [columns[i] for i in order], [names[i] for i in order])


def ref_keys(columns, names):
    """keys(): the names sorted (SparkSQLExprMapper.scala:205), the values non-null."""
    order = sorted(range(len(names)), key=lambda i: names[i])
    return ref_mask_list(MASK_NOT_NULL, [columns[i] for i in order], [names[i] for i in order])


def ref_rel_type(columns, names):
    """type(): the first TRUE flag's name in the order given, else None (get_rel_type's headOption.orNull)."""
    return [(lst[0] if lst else None) for lst in ref_mask_list(MASK_TRUE, columns, names)]
