"""Host mirror of CAPS's backend table interface over the C ABI.

``GpuTable`` follows the member names, argument meaning and error behaviour of
    trait Table[T <: Table[T]] extends CypherTable
    okapi-relational/src/main/scala/org/opencypher/okapi/relational/api/table/Table.scala:43-176
as implemented for Spark by DataFrameTable (spark-cypher/.../impl/table/SparkTable.scala:47-257),
so that a relational plan written against ``Table`` runs unchanged on the device.
Every operator executes in libcapsmi.so (HIP, gfx950); Python only marshals handles.
"""
from __future__ import annotations

import bisect
import contextlib
import ctypes
import itertools
import threading
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .expr import (BOOL, F64, I64, LIST, STR, BinOp, CapsmiExpr, Case, Col, Explode, Expr, In, Index, InList, Keys, Labels, ListLit,
                   Lit, Param, Range, Size, STRING_SYNC_OPS, contains_range, needs_list_lowering, compile_program,
                   contains_explode, mask_list_args, to_ctypes)

_TLS = threading.local()

_EXPR_PTR = ctypes.POINTER(CapsmiExpr)
_TMP_IDS = itertools.count()  # names of the temporary list columns of Range / Labels / Keys operands
_LIST_SOURCES = (Range, Labels, Keys)  # the expressions that a plan node of their own turns into a list column
_MISPLACED = "{} is a whole withColumns column or the argument of Explode / Size / Index / InList"
_LIT_PROGS = {}  # (python type, value, declared type) -> one-node program of a Boolean / Long / null literal

JOIN_TYPES = {"inner": 0, "left_outer": 1, "right_outer": 2, "full_outer": 3, "cross": 4}
AGG_KINDS = {"count_star": 0, "count": 1, "min": 2, "max": 3, "sum": 4, "avg": 5, "collect": 6}


@dataclass
class ColumnData:
    """Host column: ``values`` int64 (I64/BOOL/STR codes) or float64 (F64); ``valid`` bool mask or None.
    A list column (type LIST + element type) holds one numpy array of element words per row (object
    array; float64 elements for F64 lists)."""
    name: str
    type: int
    values: np.ndarray
    valid: Optional[np.ndarray] = None

    def words(self) -> np.ndarray:
        if self.type >= LIST:
            raise _lib.IllegalArgumentException(f"list column {self.name} has no row words; see csr()")
        v = np.asarray(self.values)
        if self.type == F64:
            return np.ascontiguousarray(v.astype(np.float64)).view(np.int64)
        return np.ascontiguousarray(v.astype(np.int64))


def _element_words(ty: int, v) -> np.ndarray:
    a = np.asarray(v)
    if ty == F64:
        return np.ascontiguousarray(a.astype(np.float64)).view(np.int64).reshape(-1)
    return np.ascontiguousarray(a.astype(np.int64)).reshape(-1)


def list_csr(c: ColumnData) -> Tuple[np.ndarray, np.ndarray]:
    """(offsets int64[n + 1], element words int64) of a list ColumnData; a null or None row is empty."""
    elem = c.type - LIST
    rows = [np.empty(0, dtype=np.int64) if (r is None or (c.valid is not None and not c.valid[i]))
            else _element_words(elem, r) for i, r in enumerate(c.values)]
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        np.cumsum([len(r) for r in rows], out=offs[1:])
    vals = np.concatenate(rows) if rows else np.empty(0, dtype=np.int64)
    return offs, np.ascontiguousarray(vals, dtype=np.int64)


def typed_values(items: Sequence[object], encode_str, what: str):
    """(element type, capsmi_value array) of Python scalars of one type (None = null); an int list with a
    float is Double; an empty or all-null list is Long."""
    from .expr import _lit_bits

    def type_of(v):
        return BOOL if isinstance(v, (bool, np.bool_)) else I64 if isinstance(v, (int, np.integer)) \
            else F64 if isinstance(v, (float, np.floating)) else STR if isinstance(v, str) else None

    for x in items:
        if x is not None and type_of(x) is None:
            raise _lib.NotImplementedException(f"{what}: value {x!r} (nested lists and maps are not supported)")
    tys = {type_of(x) for x in items} - {None}
    if tys == {I64, F64}:
        tys = {F64}
    if len(tys) > 1:
        raise _lib.IllegalArgumentException(f"{what}: mixed value types")
    ty = tys.pop() if tys else I64
    vals = (_lib.Value * max(1, len(items)))()
    for k, x in enumerate(items):
        vals[k].is_null = 1 if x is None else 0
        vals[k].ival = 0 if x is None else _lit_bits(x, ty, encode_str)
    return ty, vals


def decode_value(ty: int, v, dictionary):
    """One exported value as a Python value (CypherValue analogue); lists element by element."""
    if ty >= LIST:
        return [decode_value(ty - LIST, x, dictionary) for x in v]
    if ty == BOOL:
        return bool(v)
    if ty == STR:
        return dictionary.decode(int(v))
    if ty == F64:
        return float(v)
    return int(v)


class StringDictionary:
    """Order-preserving dictionary for CTString values (include/capsmi.h: STR columns are codes).

    Codes are stable: once a string has a code it keeps it for the life of the dictionary, so device
    columns encoded earlier (a first graph, a driving table) stay valid when later graphs or
    literals bring new strings.  Order is preserved by allocating codes from gaps: a batch of new
    strings that falls between two known neighbours is spread evenly over the open interval between
    their codes (the first batch over [-2^62, 2^62]).  Equality and ordering on codes therefore equal
    equality and ordering on strings.  Every string that is encoded -- query literals included --
    is inserted, so two distinct strings never share a code.  A gap only runs out after ~60 nested
    insertions at one spot; that raises instead of renumbering codes already on the device.

    ``growth`` counts the extensions that added a string: a caller that handed ``arrays()`` on (the session's
    string store, ``Session.sync_strings``) compares it to know whether the dictionary has grown since."""

    LO, HI = -(1 << 62), 1 << 62

    def __init__(self, strings: Iterable[str] = ()):
        self._sorted: List[str] = []
        self._codes: List[int] = []
        self._by_code = {}
        self.growth = 0
        self.extend(strings)

    def arrays(self):
        """``(codes int64[n], offsets int64[n + 1], bytes)`` of the n strings in code order -- which is string
        order: string i has code ``codes[i]`` and the UTF-8 bytes ``bytes[offsets[i]:offsets[i + 1]]`` (the arrays
        of include/capsmi.h capsmi_session_set_strings).  A string that carries bytes which are not UTF-8 as
        surrogate escapes (PEP 383, ``bytes.decode("utf-8", "surrogateescape")``) is stored as those bytes."""
        enc = [x.encode("utf-8", "surrogateescape") for x in self._sorted]
        offsets = np.zeros(len(enc) + 1, dtype=np.int64)
        if enc:
            np.cumsum([len(b) for b in enc], out=offsets[1:])
        return np.array(self._codes, dtype=np.int64), offsets, b"".join(enc)

    def extend(self, strings: Iterable[str]) -> None:
        new = sorted(set(strings) - set(self._by_code.values()))
        if not new:
            return
        # group the new strings by the gap (insertion point) they fall into
        groups = {}
        for x in new:
            groups.setdefault(bisect.bisect_left(self._sorted, x), []).append(x)
        placed = []
        for i, xs in groups.items():
            lo = self._codes[i - 1] if i > 0 else self.LO
            hi = self._codes[i] if i < len(self._codes) else self.HI
            step = (hi - lo) // (len(xs) + 1)
            if step < 1:
                raise OverflowError("string dictionary: no code left between "
                                    f"{self._sorted[i - 1] if i > 0 else None!r} and "
                                    f"{self._sorted[i] if i < len(self._sorted) else None!r}")
            placed += [(lo + (k + 1) * step, x) for k, x in enumerate(xs)]
        for c, x in placed:
            self._by_code[c] = x
        self.growth += 1
        merged = sorted(list(zip(self._codes, self._sorted)) + placed)
        self._codes = [c for c, _ in merged]
        self._sorted = [x for _, x in merged]

    def intern_batch(self, offsets, data) -> np.ndarray:
        """The codes (int64[n]) of the n strings ``data[offsets[i]:offsets[i + 1]]`` -- the arrays a string sink gets
        (include/capsmi.h capsmi_string_sink_fn): one ``extend`` for the whole batch, so ``growth`` moves at most once,
        then one lookup per string.  The strings may repeat and may be known.  Bytes that are not UTF-8 are kept as
        surrogate escapes, the inverse of ``arrays()``."""
        data = bytes(data)
        strs = [data[int(offsets[i]):int(offsets[i + 1])].decode("utf-8", "surrogateescape")
                for i in range(len(offsets) - 1)]
        self.extend(strs)
        return np.fromiter((self._codes[bisect.bisect_left(self._sorted, x)] for x in strs), dtype=np.int64,
                           count=len(strs))

    def encode(self, s: str) -> int:
        i = bisect.bisect_left(self._sorted, s)
        if i < len(self._sorted) and self._sorted[i] == s:
            return self._codes[i]
        self.extend([s])
        return self._codes[bisect.bisect_left(self._sorted, s)]

    def decode(self, code: int) -> str:
        try:
            return self._by_code[int(code)]
        except KeyError:
            raise KeyError(f"code {code} is not a dictionary string") from None

    def __len__(self) -> int:
        return len(self._sorted)


class Session:
    """One device, one HIP stream (CAPSSession.local analogue, spark-cypher/.../api/CAPSSession.scala:110-131)."""

    def __init__(self, device: int = 0, dictionary: Optional[StringDictionary] = None):
        self._h = ctypes.c_void_p()
        _lib.call("capsmi_session_create", device, ctypes.byref(self._h))
        self.device = device
        self.dictionary = dictionary or StringDictionary()
        self.params: List[object] = []  # the values of set_params (Explode of a list Param reads them)
        self._strings_at = None  # the dictionary's growth counter at the last upload of the string store
        # the string sink (include/capsmi.h capsmi_session_set_string_sink): strings made on the device get their
        # codes from this session's dictionary; the callback object lives as long as the session
        self._sink_cb = _lib.STRING_SINK_FN(self._string_sink)
        self.set_string_sink(self._sink_cb)

    def _string_sink(self, _ctx, n, offsets, data, codes_out) -> int:
        try:
            off = np.ctypeslib.as_array(offsets, shape=(n + 1,))
            synced = self._strings_at == self.dictionary.growth
            codes = self.dictionary.intern_batch(off, ctypes.string_at(data, int(off[n])))
            ctypes.memmove(codes_out, codes.ctypes.data, 8 * n)
            if synced:  # the library merges what is new into its store: nothing to upload again
                self._strings_at = self.dictionary.growth
            return 0
        except Exception:  # an exception cannot cross the C frames: the action fails with the sink's status
            return 1

    def set_string_sink(self, cb) -> None:
        """Register ``cb`` (a ``_lib.STRING_SINK_FN`` the caller keeps alive) as the session's string sink, None to
        remove it.  The session registers its dictionary's at creation."""
        _lib.call("capsmi_session_set_string_sink", self._h, cb if cb is not None else _lib.STRING_SINK_FN(), None)

    def string_count(self) -> int:
        """Entries of the string store registered on the device (capsmi_session_string_count)."""
        n = ctypes.c_int64()
        _lib.call("capsmi_session_string_count", self._h, ctypes.byref(n))
        return n.value

    @property
    def handle(self):
        return self._h

    def set_stream(self, hip_stream: Optional[int]) -> None:
        """Run on `hip_stream` (an int handle, e.g. ``torch.cuda.current_stream().cuda_stream``;
        0 is the null stream, torch's default), or on the session's own stream for None."""
        if hip_stream is None:
            _lib.call("capsmi_session_set_stream", self._h, ctypes.c_void_p(0))
        else:
            _lib.call("capsmi_session_use_stream", self._h, ctypes.c_void_p(hip_stream))

    def sync(self) -> None:
        _lib.call("capsmi_session_sync", self._h)

    def set_config(self, name: str, value: Optional[str]) -> None:
        """One CAPSMI_* knob for this session (include/capsmi.h capsmi_session_set_config); the environment is
        read only when the session is created.  None = back to the environment's value or the default."""
        _lib.call("capsmi_session_set_config", self._h, name.encode(),
                  None if value is None else str(value).encode())

    @contextlib.contextmanager
    def configured(self, **knobs):
        """``with session.configured(CAPSMI_COUNT="atomic"): ...`` -- the knobs for the block, then back to the
        environment's values (or the defaults)."""
        for k, v in knobs.items():
            self.set_config(k, v)
        try:
            yield self
        finally:
            for k in knobs:
                self.set_config(k, None)

    def close(self) -> None:
        if self._h:
            _lib.call("capsmi_session_destroy", self._h)
            self._h = ctypes.c_void_p()

    def table(self, columns: Sequence[ColumnData]) -> "GpuTable":
        """CAPSNodeTable / CAPSRelationshipTable ingest: copies host columns to the device."""
        n = len(columns[0].values) if columns else 0
        for c in columns:
            if len(c.values) != n:
                raise _lib.IllegalArgumentException(f"column {c.name} has {len(c.values)} rows, expected {n}")
        lists = [c for c in columns if c.type >= LIST]
        if lists:  # array columns: the plain columns first, each list column appended, then the given order
            t = self.table([c for c in columns if c.type < LIST]) if len(lists) < len(columns) else self._rows_only(n)
            for c in lists:
                t = t.add_list_column(c)
            return t.select(*[c.name for c in columns])
        descs = (_lib.ColDesc * max(1, len(columns)))()
        keep = []
        for i, c in enumerate(columns):
            w = c.words()
            keep.append(w)
            descs[i].name = c.name.encode()
            descs[i].type = c.type
            descs[i].data = w.ctypes.data if n else None
            if c.valid is not None:
                vb = np.ascontiguousarray(np.asarray(c.valid, dtype=np.uint8))
                keep.append(vb)
                descs[i].valid = vb.ctypes.data if n else None
            else:
                descs[i].valid = None
        out = ctypes.c_void_p()
        _lib.call("capsmi_table_from_host", self._h, len(columns), descs, n, ctypes.byref(out))
        return GpuTable(self, out)

    def _rows_only(self, n: int) -> "GpuTable":
        """A table of n rows and no column (the carrier of list columns given alone)."""
        out = ctypes.c_void_p()
        _lib.call("capsmi_table_from_host", self._h, 0, (_lib.ColDesc * 1)(), n, ctypes.byref(out))
        return GpuTable(self, out)

    def encode_str(self, s: str) -> int:
        return self.dictionary.encode(s)

    def sync_strings(self) -> None:
        """Register the dictionary's strings as the session's string store (include/capsmi.h
        capsmi_session_set_strings), which StartsWith / EndsWith / Contains, StrSize / StrToInteger / StrToFloat /
        ToBoolean and the String operands of Concat read on the device, and into which ToString / Concat merge the
        strings they make (the sink then moves ``_strings_at`` along, so they are not uploaded again).  Uploads the whole dictionary when it has grown since the last upload, else
        nothing; codes are stable, so every store is a superset of the one before and programs compiled earlier stay
        valid."""
        if self._strings_at == self.dictionary.growth:
            return
        codes, offsets, data = self.dictionary.arrays()
        _lib.call("capsmi_session_set_strings", self._h, len(codes), codes.ctypes.data, offsets.ctypes.data, data)
        self._strings_at = self.dictionary.growth

    def read_csv(self, paths: Sequence[str], names: Sequence[str], types: Sequence[int], delimiter: Optional[str] = ",",
                 comment: Optional[str] = None, row_id_col: Optional[str] = None) -> "GpuTable":
        """DataFrameReader.csv with an explicit schema, parsed natively by host threads into a device
        table (include/capsmi.h capsmi_read_csv).  ``delimiter`` is Spark's one-character ``sep``;
        None opts in to whitespace splitting (runs of blanks).  String fields are encoded with this
        session's dictionary."""
        def intern(_ctx, ptr, n):
            return self.dictionary.encode(ctypes.string_at(ptr, n).decode("utf-8"))

        cb = _lib.INTERN_FN(intern)
        tys = (ctypes.c_int32 * max(1, len(types)))(*types)
        out = ctypes.c_void_p()
        _lib.call("capsmi_read_csv", self._h, len(paths), _lib.strs(list(paths)),
                  b"\0" if delimiter is None else delimiter.encode()[:1],
                  (comment or "\0").encode()[:1], len(names), _lib.strs(list(names)), tys, cb, None,
                  row_id_col.encode() if row_id_col else None, ctypes.byref(out))
        return GpuTable(self, out)

    def compact_graph(self, nodes: Sequence["GpuTable"], rels: Sequence["GpuTable"]) -> int:
        """Dense ids for one graph's registered node / relationship tables (include/capsmi.h
        capsmi_graph_compact); returns the number of dense ids."""
        na = (ctypes.c_void_p * max(1, len(nodes)))(*[t.handle for t in nodes])
        ra = (ctypes.c_void_p * max(1, len(rels)))(*[t.handle for t in rels])
        n = ctypes.c_int64()
        _lib.call("capsmi_graph_compact", self._h, len(nodes), na, len(rels), ra, ctypes.byref(n))
        return n.value

    def compact_if_sparse(self, nodes: Sequence["GpuTable"], rels: Sequence["GpuTable"]) -> bool:
        """Compact when the tables' ids do not fit the fused kernels' window of 2^30 ids."""
        spans = [t.entity() for t in list(nodes) + list(rels)]
        spans = [(lo, hi) for k, lo, hi in spans if k and hi > lo]
        if not spans or max(h for _, h in spans) - min(l for l, _ in spans) <= (1 << 30):
            return False
        self.compact_graph(nodes, rels)
        return True

    def set_params(self, values: Sequence[object]) -> None:
        """Query parameters for ``expr.Param(i)`` (the CypherMap of SparkSQLExprMapper.scala:86-92):
        ``values[i]`` is a Python scalar (int, float, bool, str, None) or a list of them (usable as the
        element list of ``In``).  Strings are dictionary-encoded; an int list with a float is Double."""
        from .expr import BOOL, F64, I64, STR, _lit_bits

        def type_of(v):
            return BOOL if isinstance(v, bool) else I64 if isinstance(v, int) else F64 if isinstance(v, float) \
                else STR if isinstance(v, str) else None

        self.params = list(values)
        keep, arr = [], (_lib.Param * max(1, len(values)))()
        for i, v in enumerate(values):
            items = list(v) if isinstance(v, (list, tuple)) else [v]
            tys = {type_of(x) for x in items} - {None}
            if tys == {I64, F64}:
                tys = {F64}
            if len(tys) > 1:
                raise _lib.IllegalArgumentException(f"parameter {i}: mixed value types")
            ty = tys.pop() if tys else I64
            vals = (_lib.Value * max(1, len(items)))()
            for k, x in enumerate(items):
                vals[k].is_null = 1 if x is None else 0
                vals[k].ival = 0 if x is None else _lit_bits(x, ty, self.encode_str)
            keep.append(vals)
            arr[i].type, arr[i].is_list, arr[i].count, arr[i].values = ty, int(isinstance(v, (list, tuple))), \
                len(items), ctypes.cast(vals, ctypes.c_void_p)
        _lib.call("capsmi_session_set_params", self._h, len(values), arr)

    def set_fused(self, enabled: bool) -> None:
        """Route lazy plans of the Expand shapes to the fused kernels (default) or run them operator
        by operator (include/capsmi.h capsmi_session_set_fused)."""
        _lib.call("capsmi_session_set_fused", self._h, 1 if enabled else 0)

    def set_unrouted_limit(self, max_bytes: int) -> None:
        """Refuse unrouted joins whose estimated output exceeds `max_bytes` (0: no limit;
        include/capsmi.h capsmi_session_set_unrouted_limit)."""
        _lib.call("capsmi_session_set_unrouted_limit", self._h, int(max_bytes))

    def set_csv_partitioning(self, default_parallelism: int, max_partition_bytes: int = 128 << 20,
                             open_cost_bytes: int = 4 << 20) -> None:
        """read_csv row ids as Spark's monotonically_increasing_id over its file-scan partitions
        (include/capsmi.h capsmi_session_set_csv_partitioning); 0 = one partition (row numbers)."""
        _lib.call("capsmi_session_set_csv_partitioning", self._h, int(default_parallelism), int(max_partition_bytes),
                  int(open_cost_bytes))

    def set_ranks(self, rank: int, world: int, collective=None) -> None:
        """This process is rank `rank` of `world`; `collective(op, send_ptr, recv_ptr, count, dtype)`
        runs the exchange on this session's stream (capsmi.dist.TorchCollective; include/capsmi.h
        capsmi_session_set_ranks)."""
        if collective is None:
            self._coll = None
            _lib.call("capsmi_session_set_ranks", self._h, rank, world, _lib.COLLECTIVE_FN(), None)
            return

        def fn(_ctx, op, send, recv, count, dtype):
            try:
                collective(op, send, recv, count, dtype)
                return 0
            except Exception as e:  # reported as CAPSMI_ERR_DEVICE by the library
                self.collective_error = e
                return 1

        self._coll = _lib.COLLECTIVE_FN(fn)  # kept alive with the session
        _lib.call("capsmi_session_set_ranks", self._h, rank, world, self._coll, None)

    def route_count(self, name: str) -> int:
        """Plans routed to fused entry point `name` ("expand", "expand_count", "two_hop", "triangle",
        "triangle_grouped", "triangle_transitive", "triangle_transitive_grouped", "triangle_undirected", "triangle_undirected_grouped", "var_length", "var_length_distinct") so far; "miss" counts materialisations where a pattern ran unrouted."""
        v = ctypes.c_int64()
        _lib.call("capsmi_session_route_count", self._h, name.encode(), ctypes.byref(v))
        return v.value


class GpuTable:
    """A device-resident, immutable table; each operator returns a new GpuTable."""

    def __init__(self, session: Session, handle: ctypes.c_void_p):
        self.session = session
        self._h = handle
        self._schema = None  # (names, types): tables are immutable, so the schema is read once
        self._index = None  # name -> position (expression compilation)
        self._leaf = None  # column name -> its one-node program (the planner's scans project columns)
        self._wcols = None  # withColumns argument arrays of column / literal projections, by structure

    # ---- lifetime ------------------------------------------------------------------------
    @property
    def handle(self):
        return self._h

    def release(self) -> None:
        if self._h:
            _lib.call("capsmi_table_release", self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            if self._h and _lib._lib is not None:
                _lib._lib.capsmi_table_release(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass

    def _wrap(self, h) -> "GpuTable":
        return GpuTable(self.session, h)

    # ---- CypherTable (okapi-api/.../api/table/CypherTable.scala:41-68) -------------------
    @property
    def size(self) -> int:
        v = ctypes.c_int64()
        _lib.call("capsmi_table_size", self._h, ctypes.byref(v))
        return v.value

    _MAXC = 256

    def _read_schema(self):
        if self._schema is None:  # one call for names and types (include/capsmi.h capsmi_table_schema)
            n = ctypes.c_int32()
            buf = getattr(_TLS, "names", None)  # a reusable name buffer per thread (ctypes drops the GIL)
            if buf is None:
                buf = _TLS.names = ctypes.create_string_buffer(16384)
            types = (ctypes.c_int32 * self._MAXC)()
            _lib.call("capsmi_table_schema", self._h, ctypes.byref(n), buf, len(buf), types, None, self._MAXC)
            if n.value > self._MAXC:
                raise _lib.NotImplementedException(f"table with {n.value} columns")
            raw, names, pos = buf.raw, [], 0  # n NUL-terminated names (not a split of the whole buffer)
            for _ in range(n.value):
                end = raw.index(b"\0", pos)
                names.append(raw[pos:end].decode())
                pos = end + 1
            self._schema = (names, list(types[:n.value]))
        return self._schema

    @property
    def physicalColumns(self) -> List[str]:
        return list(self._read_schema()[0])

    @property
    def columnType(self) -> dict:
        names, types = self._read_schema()
        return dict(zip(names, types))

    # ---- entity tables (include/capsmi.h capsmi_node_table / capsmi_rel_table) -----------------
    def as_node_table(self, id_col: str, label_cols: Sequence[str] = ()) -> "GpuTable":
        """CAPSNodeTable + EntityTable.verify (EntityTable.scala:59-65, 105-131)."""
        out = ctypes.c_void_p()
        _lib.call("capsmi_node_table", self._h, id_col.encode(), len(label_cols), _lib.strs(label_cols),
                  ctypes.byref(out))
        return self._wrap(out)

    def as_rel_table(self, id_col: str, src_col: str, dst_col: str, type_cols: Sequence[str] = ()) -> "GpuTable":
        """CAPSRelationshipTable + EntityTable.verify (EntityTable.scala:59-65, 137-164)."""
        out = ctypes.c_void_p()
        _lib.call("capsmi_rel_table", self._h, id_col.encode(), src_col.encode(), dst_col.encode(), len(type_cols),
                  _lib.strs(type_cols), ctypes.byref(out))
        return self._wrap(out)

    @property
    def partitioned(self) -> bool:
        """Whether the rows are this rank's partition of a distributed result."""
        v = ctypes.c_int32()
        _lib.call("capsmi_table_partitioned", self._h, ctypes.byref(v))
        return bool(v.value)

    def owned_rows(self, col: str, id_lo: int, id_hi: int) -> "GpuTable":
        """The rows whose Long column `col` holds an id this rank owns (include/capsmi.h capsmi_owned_rows)."""
        out = ctypes.c_void_p()
        _lib.call("capsmi_owned_rows", self.session.handle, self._h, col.encode(), id_lo, id_hi, ctypes.byref(out))
        return self._wrap(out)

    def entity(self) -> Tuple[int, int, int]:
        """(kind: 0 plain / 1 node / 2 relationship, id_lo, id_hi)"""
        k, lo, hi = ctypes.c_int32(), ctypes.c_int64(), ctypes.c_int64()
        _lib.call("capsmi_table_entity", self._h, ctypes.byref(k), ctypes.byref(lo), ctypes.byref(hi))
        return k.value, lo.value, hi.value

    def flatten_rel_types(self, type_col: str, types: Sequence[str], out_cols: Sequence[str]) -> "GpuTable":
        """CAPSRelationshipTable.fromMapping's String type column -> Boolean flags (CAPSTable.scala:189-204)."""
        codes = (ctypes.c_int64 * max(1, len(types)))(*[self.session.encode_str(t) for t in types])
        out = ctypes.c_void_p()
        _lib.call("capsmi_flatten_rel_types", self._h, type_col.encode(), len(types), codes, _lib.strs(out_cols),
                  ctypes.byref(out))
        return self._wrap(out)

    def column_index(self, name: str) -> int:
        v = ctypes.c_int32()
        _lib.call("capsmi_table_column_index", self._h, name.encode(), ctypes.byref(v))
        if v.value < 0:
            raise _lib.IllegalArgumentException(f"no column named '{name}'")
        return v.value

    def column(self, name: str, offset: int = 0, n: Optional[int] = None) -> ColumnData:
        idx = self.column_index(name)
        size = self.size
        if n is None:
            n = size - offset
        ty = self.columnType[name]
        if ty >= LIST:
            return self._list_column(name, idx, ty, offset, n)
        vals = np.empty(n, dtype=np.int64)
        valid = np.empty(n, dtype=np.uint8)
        _lib.call("capsmi_table_export", self._h, idx, vals.ctypes.data if n else None,
                  valid.ctypes.data if n else None, offset, n)
        nullable = ctypes.c_int32()
        _lib.call("capsmi_table_column_nullable", self._h, idx, ctypes.byref(nullable))
        if ty == F64:
            vals = vals.view(np.float64)
        return ColumnData(name, ty, vals, valid.astype(bool) if nullable.value else None)

    def _list_column(self, name: str, idx: int, ty: int, offset: int, n: int) -> ColumnData:
        """A list column's rows (include/capsmi.h capsmi_table_export_list)."""
        total = ctypes.c_int64()
        _lib.call("capsmi_table_export_list", self._h, idx, offset, n, None, None, None, 0, ctypes.byref(total))
        offs = np.empty(n + 1, dtype=np.int64)
        valid = np.empty(max(1, n), dtype=np.uint8)
        vals = np.empty(max(1, total.value), dtype=np.int64)
        _lib.call("capsmi_table_export_list", self._h, idx, offset, n, offs.ctypes.data, valid.ctypes.data,
                  vals.ctypes.data, len(vals), ctypes.byref(total))
        if ty - LIST == F64:
            vals = vals.view(np.float64)
        rows = np.empty(n, dtype=object)
        for i in range(n):
            rows[i] = vals[offs[i]:offs[i + 1]]
        nullable = ctypes.c_int32()
        _lib.call("capsmi_table_column_nullable", self._h, idx, ctypes.byref(nullable))
        return ColumnData(name, ty, rows, valid[:n].astype(bool) if nullable.value else None)

    def to_columns(self) -> List[ColumnData]:
        return [self.column(c) for c in self.physicalColumns]

    def rows(self) -> List[dict]:
        """CypherTable.rows: host rows with strings decoded."""
        cols = self.to_columns()
        n = self.size
        out = []
        for r in range(n):
            row = {}
            for c in cols:
                if c.valid is not None and not c.valid[r]:
                    row[c.name] = None
                    continue
                row[c.name] = decode_value(c.type, c.values[r], self.session.dictionary)
            out.append(row)
        return out

    def fingerprint(self, cols: Sequence[str]) -> Tuple[int, int, int]:
        cnt, s, x = ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.call("capsmi_table_fingerprint", self._h, len(cols), _lib.strs(cols), ctypes.byref(cnt),
                  ctypes.byref(s), ctypes.byref(x))
        return cnt.value, s.value, x.value

    # ---- Table[T] operators ----------------------------------------------------------------
    def cache(self) -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_cache", self._h, ctypes.byref(out))
        return self._wrap(out)

    def select(self, *cols: str) -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_select", self._h, len(cols), _lib.strs(cols), ctypes.byref(out))
        return self._wrap(out)

    def _column_index(self) -> dict:
        if self._index is None:  # name -> position, built once per table (expressions are compiled per column)
            self._index = {n: i for i, n in enumerate(self._read_schema()[0])}
        return self._index

    def _program(self, e: Expr):
        if type(e) is Col:  # the common leaf: one program per (table, column), reused (C copies it)
            if self._leaf is None:
                self._leaf = {}
            hit = self._leaf.get(e.name)
            if hit is not None:
                return 1, hit
        elif type(e) is Lit and (e.value is None or type(e.value) in (bool, int)):  # label flags, nulls
            key = (type(e.value), e.value, e.type)
            hit = _LIT_PROGS.get(key)
            if hit is None:
                hit = _LIT_PROGS[key] = to_ctypes(compile_program(e, None, None))
            return 1, hit
        index = self._column_index()

        def col(name: str) -> int:
            if name not in index:
                raise _lib.IllegalArgumentException(f"expression references unknown column '{name}'")
            return index[name]

        prog = compile_program(e, col, self.session.encode_str)
        if any(p[0] in STRING_SYNC_OPS for p in prog):  # the literals are encoded by now: the store holds them
            self.session.sync_strings()
        arr = to_ctypes(prog)
        if type(e) is Col:
            self._leaf[e.name] = arr
        return len(prog), arr

    def filter(self, expr: Expr) -> "GpuTable":
        if type(expr) is not Col and needs_list_lowering(expr):
            if isinstance(expr, _LIST_SOURCES):  # a list is no predicate
                raise _lib.NotImplementedException(_MISPLACED.format(type(expr).__name__))
            e, temps = self._lower_lists(expr)
            if temps:  # Range / Labels / Keys operands: temporary list columns, dropped again
                t = self
                for tmp, src in temps:
                    t = t._with_list_source(src, tmp)
                return t._filter(e).drop(*[tmp for tmp, _ in temps])
            expr = e
        return self._filter(expr)

    def _filter(self, expr: Expr) -> "GpuTable":
        n, prog = self._program(expr)
        out = ctypes.c_void_p()
        _lib.call("capsmi_filter", self._h, n, prog, ctypes.byref(out))
        return self._wrap(out)

    def drop(self, *cols: str) -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_drop", self._h, len(cols), _lib.strs(cols), ctypes.byref(out))
        return self._wrap(out)

    def join(self, other: "GpuTable", join_type: str, *join_cols: Tuple[str, str]) -> "GpuTable":
        if join_type not in JOIN_TYPES:
            raise _lib.IllegalArgumentException(f"join type {join_type}")
        out = ctypes.c_void_p()
        lc = [a for a, _ in join_cols]
        rc = [b for _, b in join_cols]
        _lib.call("capsmi_join", self._h, other._h, JOIN_TYPES[join_type], len(join_cols), _lib.strs(lc),
                  _lib.strs(rc), ctypes.byref(out))
        return self._wrap(out)

    def unionAll(self, other: "GpuTable") -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_union_all", self._h, other._h, ctypes.byref(out))
        return self._wrap(out)

    def orderBy(self, *items: Tuple[str, str]) -> "GpuTable":
        cols = [c for c, _ in items]
        desc = (ctypes.c_int32 * max(1, len(items)))(*[1 if o.lower().startswith("desc") else 0 for _, o in items])
        out = ctypes.c_void_p()
        _lib.call("capsmi_order_by", self._h, len(items), _lib.strs(cols), desc, ctypes.byref(out))
        return self._wrap(out)

    def skip(self, n: int) -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_skip", self._h, n, ctypes.byref(out))
        return self._wrap(out)

    def limit(self, n: int) -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_limit", self._h, n, ctypes.byref(out))
        return self._wrap(out)

    def distinct(self, *cols: str) -> "GpuTable":
        out = ctypes.c_void_p()
        if cols:  # DataFrameTable.distinct(cols) = dropDuplicates(cols), SparkTable.scala:234-235
            _lib.call("capsmi_distinct_on", self._h, len(cols), _lib.strs(cols), ctypes.byref(out))
        else:
            _lib.call("capsmi_distinct", self._h, ctypes.byref(out))
        return self._wrap(out)

    def group(self, by: Sequence[str], aggregations: Sequence[Tuple[str, Optional[str], bool, str]]) -> "GpuTable":
        """``aggregations``: (kind, input column, distinct, output column); kind in AGG_KINDS."""
        aggs = (_lib.Agg * max(1, len(aggregations)))()
        for i, (kind, inp, distinct, outname) in enumerate(aggregations):
            aggs[i].kind = AGG_KINDS[kind]
            aggs[i].distinct = 1 if distinct else 0
            aggs[i].input = inp.encode() if inp else None
            aggs[i].output = outname.encode()
        out = ctypes.c_void_p()
        _lib.call("capsmi_group", self._h, len(by), _lib.strs(by), len(aggregations), aggs, ctypes.byref(out))
        return self._wrap(out)

    def explode(self, list_col: str, item: str) -> "GpuTable":
        """UNWIND of a list column: one row per element, none for a null or empty list; the input columns
        plus `item` (include/capsmi.h capsmi_explode).  Rows come in (input row, element position) order."""
        out = ctypes.c_void_p()
        _lib.call("capsmi_explode", self._h, list_col.encode(), item.encode(), ctypes.byref(out))
        return self._wrap(out)

    def explodeValues(self, values: Sequence[object], item: str) -> "GpuTable":
        """UNWIND of a literal list or list parameter: every row once per value (include/capsmi.h
        capsmi_explode_values).  Values are Python scalars of one type, None for null."""
        ty, vals = typed_values(list(values), self.session.encode_str, "explodeValues")
        out = ctypes.c_void_p()
        _lib.call("capsmi_explode_values", self._h, ty, len(values), ctypes.cast(vals, ctypes.c_void_p), item.encode(),
                  ctypes.byref(out))
        return self._wrap(out)

    def add_list_column(self, c: ColumnData) -> "GpuTable":
        """This table plus the list column `c` (type LIST + element type; one array of elements per row;
        include/capsmi.h capsmi_table_add_list_column)."""
        if c.type < LIST:
            raise _lib.IllegalArgumentException(f"column {c.name} is not a list column")
        offs, vals = list_csr(c)
        return self.add_list_column_csr(c.name, c.type - LIST, offs, vals, c.valid)

    def add_list_column_csr(self, name: str, elem_type: int, offsets, values, valid=None) -> "GpuTable":
        """The same from CSR arrays: `offsets` int64[rows + 1], `values` the element words."""
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if len(offs) != self.size + 1:
            raise _lib.IllegalArgumentException(f"list column {name}: {len(offs)} offsets for {self.size} rows")
        vals = np.ascontiguousarray(values)
        vals = vals.view(np.int64) if vals.dtype == np.float64 else np.ascontiguousarray(vals, dtype=np.int64)
        if len(vals) < int(offs[-1]):
            raise _lib.IllegalArgumentException(f"list column {name}: offsets end at {int(offs[-1])}, {len(vals)} values")
        vb = None if valid is None else np.ascontiguousarray(np.asarray(valid, dtype=np.uint8))
        out = ctypes.c_void_p()
        _lib.call("capsmi_table_add_list_column", self._h, name.encode(), elem_type, offs.ctypes.data,
                  vals.ctypes.data if len(vals) else None, None if vb is None or not len(vb) else vb.ctypes.data,
                  ctypes.byref(out))
        return self._wrap(out)

    def _explode_column(self, e: Explode, name: str) -> "GpuTable":
        a = e.arg
        if isinstance(a, Col):
            return self.explode(a.name, name)
        if isinstance(a, ListLit):
            return self.explodeValues(a.values, name)
        if isinstance(a, Param):
            params = self.session.params
            if not 0 <= a.index < len(params) or not isinstance(params[a.index], (list, tuple)):
                raise _lib.IllegalArgumentException(f"Explode: parameter {a.index} is not a list parameter")
            return self.explodeValues(params[a.index], name)
        raise _lib.NotImplementedException(f"Explode of {a!r}: a list column, ListLit or list Param")

    def withRangeColumn(self, start, end, step, name: str) -> "GpuTable":
        """This table plus the Long list column `name` = range(start, end, step) per row (include/capsmi.h
        capsmi_with_range_column): Long expressions or Python ints; `step` None is 1."""
        as_expr = lambda x: x if isinstance(x, Expr) else Lit(x)  # noqa: E731
        progs = [self._program(as_expr(x)) for x in (start, end)]
        progs.append((0, None) if step is None else self._program(as_expr(step)))
        args = []
        for n, prog in progs:
            args += [n, None if prog is None else ctypes.cast(prog, _EXPR_PTR)]
        out = ctypes.c_void_p()
        _lib.call("capsmi_with_range_column", self._h, *args, name.encode(), ctypes.byref(out))
        return self._wrap(out)

    def withMaskListColumn(self, mode: int, cols: Sequence[str], names: Sequence[str], name: str) -> "GpuTable":
        """This table plus the String list column `name`: per row the names[i], in the order given, whose column
        cols[i] passes -- non-null and TRUE (mode expr.MASK_TRUE, labels()) or non-null (expr.MASK_NOT_NULL,
        keys()); include/capsmi.h capsmi_with_mask_list_column.  The names go through the session dictionary."""
        if len(cols) != len(names):
            raise _lib.IllegalArgumentException(f"{len(cols)} columns for {len(names)} names")
        self.session.dictionary.extend(names)
        codes = (ctypes.c_int64 * max(1, len(names)))(*[self.session.encode_str(x) for x in names])
        out = ctypes.c_void_p()
        _lib.call("capsmi_with_mask_list_column", self._h, mode, len(cols), _lib.strs(list(cols)), codes, name.encode(),
                  ctypes.byref(out))
        return self._wrap(out)

    def _with_list_source(self, src: Expr, name: str) -> "GpuTable":
        """Column `name` = the list a Range / Labels / Keys stands for (one plan node each)."""
        if isinstance(src, Range):
            return self.withRangeColumn(src.start, src.end, src.step, name)
        return self.withMaskListColumn(*mask_list_args(src), name)

    def _lower_lists(self, e: Expr):
        """The list expressions the library does not take as they are, rewritten: InList over a ListLit or a
        list Param is the plain In; Size(ListLit) is a literal; a Range, Labels or Keys under Explode / Size /
        Index / InList becomes a reference to a temporary list column.  Returns (expression, [(temporary name,
        the Range / Labels / Keys)])."""
        temps = []

        def as_list(a: Expr) -> Expr:
            if isinstance(a, _LIST_SOURCES):
                if isinstance(a, Range):
                    check_range(a)
                tmp = f"__list_{next(_TMP_IDS)}"
                temps.append((tmp, a))
                return Col(tmp)
            return go(a)

        def check_range(r: Range) -> None:
            for x in (r.start, r.end, r.step):
                if isinstance(x, Expr) and (contains_range(x) or contains_explode(x)):
                    raise _lib.NotImplementedException("Range nested in a Range operand")

        def go(x):
            if isinstance(x, _LIST_SOURCES):
                raise _lib.NotImplementedException(_MISPLACED.format(type(x).__name__))
            if isinstance(x, Index) and not needs_list_lowering(x) and not isinstance(x.list, (ListLit, Lit)):
                return x
            if isinstance(x, InList):
                if isinstance(x.list, ListLit):
                    return In(go(x.arg), tuple(Lit(v) for v in x.list.values))
                if isinstance(x.list, Param):
                    return In(go(x.arg), (x.list,))
                if isinstance(x.list, Lit) and x.list.value is None:
                    return Lit(None, BOOL)
                return InList(go(x.arg), as_list(x.list))
            if isinstance(x, Size):
                if isinstance(x.arg, ListLit):
                    return Lit(len(x.arg.values))
                if isinstance(x.arg, Lit) and x.arg.value is None:
                    return Lit(None, I64)
                if (isinstance(x.arg, Lit) and isinstance(x.arg.value, str)) or (
                        isinstance(x.arg, Col) and self.columnType.get(x.arg.name) == STR):
                    raise _lib.NotImplementedException(
                        "size() of a string is not implemented: string lengths live in the caller's dictionary")
                return Size(as_list(x.arg))
            if isinstance(x, Index):
                if isinstance(x.list, ListLit):  # a literal list: the element whose position the index equals
                    i = go(x.index)
                    return Case(tuple((BinOp("=", i, Lit(k)), Lit(v)) for k, v in enumerate(x.list.values)))
                if isinstance(x.list, Lit) and x.list.value is None:
                    return Lit(None)
                return Index(as_list(x.list), go(x.index))
            if isinstance(x, Explode):
                return Explode(as_list(x.arg))
            if not isinstance(x, Expr) or isinstance(x, (Col, Lit, Param, ListLit)):
                return x
            kw = {}
            for k, v in x.__dict__.items():
                if isinstance(v, tuple):
                    v = tuple(tuple(go(y) for y in w) if isinstance(w, tuple) else go(w) for w in v)
                kw[k] = go(v) if isinstance(v, Expr) else v
            return type(x)(**kw)

        if isinstance(e, _LIST_SOURCES):  # the whole column
            if isinstance(e, Range):
                check_range(e)
            return e, temps
        return go(e), temps

    def _with_list_columns(self, columns) -> "GpuTable":
        """withColumns with Range / Labels / Keys / Size / Index / InList among the expressions (see
        _lower_lists).  A column that is a Range, Labels or Keys splits the call, as an Explode does: the columns
        before it are evaluated first, the ones after it see it."""
        t, drop, batch = self, [], []
        for e, name in columns:
            e, temps = t._lower_lists(e)
            if temps or isinstance(e, _LIST_SOURCES + (Explode,)):
                if batch:
                    t, batch = t._with_columns(batch), []
                for tmp, src in temps:
                    t = t._with_list_source(src, tmp)
                    drop.append(tmp)
            if isinstance(e, _LIST_SOURCES):
                t = t._with_list_source(e, name)
            elif temps or isinstance(e, Explode):
                t = t._with_columns(((e, name),))
            else:
                batch.append((e, name))
        if batch:
            t = t._with_columns(batch)
        return t.drop(*drop) if drop else t

    def withColumns(self, *columns: Tuple[Expr, str]) -> "GpuTable":
        if any(type(e) is not Col and type(e) is not Lit and needs_list_lowering(e) for e, _ in columns):
            if sum(1 for e, _ in columns if contains_explode(e)) > 1:
                raise _lib.NotImplementedException("more than one Explode in one withColumns")
            return self._with_list_columns(columns)
        return self._with_columns(columns)

    def _with_columns(self, columns) -> "GpuTable":
        gen = [i for i, (e, _) in enumerate(columns) if contains_explode(e)]
        if gen:  # UNWIND: Explode(list) AS item (RelationalPlanner.scala:94-96); one generator per call
            if len(gen) > 1:
                raise _lib.NotImplementedException("more than one Explode in one withColumns")
            e, name = columns[gen[0]]
            if not isinstance(e, Explode) or contains_explode(e.arg):
                raise _lib.NotImplementedException("Explode nested in another expression")
            t = self.withColumns(*columns[:gen[0]]) if gen[0] else self
            t = t._explode_column(e, name)
            rest = columns[gen[0] + 1:]
            return t.withColumns(*rest) if rest else t
        # the scans' projections (columns and label / null literals) repeat on the same entity tables
        # query after query: their argument arrays are kept per table, keyed by their structure
        key = []
        for e, name in columns:
            if type(e) is Col:
                key.append((name, e.name))
            elif type(e) is Lit and (e.value is None or type(e.value) in (bool, int)):
                key.append((name, type(e.value), e.value, e.type))
            else:
                key = None
                break
        if key is not None:
            key = tuple(key)
            hit = self._wcols.get(key) if self._wcols is not None else None
            if hit is not None:
                out = ctypes.c_void_p()
                _lib.call("capsmi_with_columns", self._h, len(columns), hit[0], ctypes.byref(out))
                return self._wrap(out)
        arr = (_lib.ExprColumn * max(1, len(columns)))()
        keep = []
        for i, (e, name) in enumerate(columns):
            n, prog = self._program(e)
            keep.append(prog)
            arr[i].name = name.encode()
            arr[i].nnodes = n
            arr[i].prog = ctypes.cast(prog, _EXPR_PTR)
        if key is not None:
            if self._wcols is None or len(self._wcols) > 256:
                self._wcols = {}
            self._wcols[key] = (arr, keep)  # keep: the programs the array points into
        out = ctypes.c_void_p()
        _lib.call("capsmi_with_columns", self._h, len(columns), arr, ctypes.byref(out))
        return self._wrap(out)

    def withColumnRenamed(self, old: str, new: str) -> "GpuTable":
        out = ctypes.c_void_p()
        _lib.call("capsmi_with_column_renamed", self._h, old.encode(), new.encode(), ctypes.byref(out))
        return self._wrap(out)

    def show(self, rows: int = 20) -> None:
        for r in self.limit(rows).rows():
            print(r)
