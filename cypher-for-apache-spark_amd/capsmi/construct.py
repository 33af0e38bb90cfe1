"""CONSTRUCT: graphs built from query results, their new ids made on the device.

Restates, over the ``Table`` operators of capsmi.table.GpuTable,
  - ConstructGraphPlanner.planConstructGraph / planConstructEntities / computeNodeProjections /
    computeRelationshipProjections / generateId (okapi-relational/.../impl/planning/ConstructGraphPlanner.scala:52-272)
  - SingleTableGraph.scanOperator (okapi-relational/.../impl/graph/SingleTableGraph.scala:49-106), here ``PatternGraph``.

The mirror has no Cypher front end, so a construct clause is what the front end hands the relational planner
(LogicalPatternGraph), with implicit clones already listed (IRBuilder's work):

    {"on": [graph names], "clones": [[alias, original], ...],
     "creates": [{"node": v, "labels": [...], "copy_of": base?},
                 {"rel": r, "src": a, "dst": b, "type": T?, "copy_of": base?}, ...],
     "sets": [["prop", v, key, <expr spec>], ["label", v, [labels]]]}

Column naming is the planner's: node v -> "v", "v:Label", "v.key"; relationship r -> "r", "r.__src", "r.__dst",
"r.__type" (one String column where the reference keeps a flag per type), "r.key".

Generated ids are ``set_tag(MonotonicallyIncreasingId() + (k << (33 - (floor(ln n) + 1))), tag)``: the row index is
CAPSMI_X_ROW_ID, whose withColumns node the plan executor pins (include/capsmi.h), so the ids a relationship's endpoints
copy are the ids the node scan sees.  Distributed sessions refuse the node when it is built.
"""
from __future__ import annotations

import math
from typing import Dict, List, Mapping, Sequence, Set, Tuple

import numpy as np

from .expr import (BOOL, F64, I64, STR, Case, Coalesce, Col, Expr, In, IsNotNull, BinOp, Lit, MonotonicallyIncreasingId, Not,
                   ands)
from .tagging import compute_retaggings, expr_replace_tags, expr_set_tag, pick_free_tag

TOTAL_ID_SPACE_BITS = 33  # generateId: "The first half of the id space is protected"


def _planner():
    from . import planner  # planner imports this module's entry points lazily too
    return planner


# ---- generateId -----------------------------------------------------------------------------------------
def id_offset(k: int, n: int) -> int:
    """columnPartitionOffset of created entity ``k`` of ``n`` (ConstructGraphPlanner.scala:261-270).  ``math.log`` is
    the natural logarithm, as in the reference: restated, not fixed."""
    bits = int(math.floor(math.log(n))) + 1
    return k << (TOTAL_ID_SPACE_BITS - bits)


def generate_id(k: int, n: int) -> Expr:
    return BinOp("+", MonotonicallyIncreasingId(), Lit(id_offset(k, n)))


# ---- tags -----------------------------------------------------------------------------------------------
def tag_strategy(on: Sequence[Tuple[object, Set[int]]], match: Sequence[Tuple[object, Set[int]]]):
    """(the ON plan's tag strategy, constructTagStrategy) for ON graphs and match graphs given as (key, tags) in
    order.  The ON plan retags its graphs against each other (Start's computeRetaggings of one graph,
    GraphUnionAll's of several); the construct strategy keeps those fixed and fits the match graphs in after them
    (:55-76) -- ON graphs first, which the reference's tests pin."""
    on_strategy = compute_retaggings({k: set(t) for k, t in on})
    graphs: Dict[object, Set[int]] = {k: set(t) for k, t in on}
    for k, t in match:
        graphs.setdefault(k, set(t))
    return on_strategy, compute_retaggings(graphs, on_strategy)


# ---- the header's variables -------------------------------------------------------------------------------
def owned(header: Sequence[str], v: str) -> List[str]:
    """The columns variable ``v`` owns (RecordHeader.ownedBy)."""
    return [h for h in header if h == v or h.startswith(v + ".") or h.startswith(v + ":")]


def _id_cols(v: str, is_rel: bool) -> List[str]:
    return [v, f"{v}.__src", f"{v}.__dst"] if is_rel else [v]


# ---- validation --------------------------------------------------------------------------------------------
def validate(spec: dict, node_vars: Set[str], rel_vars: Set[str]) -> None:
    """What the front end would have refused: every message names the variable."""
    PlanningError = _planner().PlanningError
    bound = set(node_vars) | set(rel_vars)
    clones = [tuple(c) for c in spec.get("clones", [])]
    for alias, orig in clones:
        if orig not in bound:
            raise PlanningError(f"unknown clone original {orig} (CLONE {orig} AS {alias})")
    names = [a for a, _ in clones]
    if len(set(names)) != len(names):
        raise PlanningError("a variable is cloned twice under one name")
    cloned_nodes = {a for a, o in clones if o in node_vars}
    cloned_rels = {a for a, o in clones if o in rel_vars}
    created_nodes, created_rels = set(), set()
    for c in spec.get("creates", []):
        if "node" in c:
            created_nodes.add(c["node"])
    for c in spec.get("creates", []):
        base = c.get("copy_of")
        if "node" in c:
            if base is not None and base not in node_vars:
                raise PlanningError(f"copy_of {base}: no such node variable (COPY OF for {c['node']})")
        elif "rel" in c:
            for end in (c["src"], c["dst"]):
                if end not in cloned_nodes | created_nodes:
                    raise PlanningError(f"endpoint {end} of created relationship {c['rel']} is neither cloned nor created")
            if base is not None and base not in rel_vars:
                raise PlanningError(f"copy_of {base}: no such relationship variable (COPY OF for {c['rel']})")
            if base is None and c.get("type") is None and c["rel"] not in cloned_rels:  # a cloned one is not created
                raise PlanningError(f"created relationship {c['rel']} has neither a type nor a base relationship")
            created_rels.add(c["rel"])
        else:
            raise PlanningError(f"a created entity is a node or a rel: {c!r}")
    kept_nodes = cloned_nodes | created_nodes
    kept = kept_nodes | cloned_rels | created_rels
    for s in spec.get("sets", []):
        if s[0] not in ("prop", "label"):
            raise PlanningError(f"unknown SET item {s!r}")
        if s[1] not in kept:
            raise PlanningError(f"SET on a dropped variable {s[1]}: it is neither cloned nor created")
        if s[0] == "label" and s[1] not in kept_nodes:
            raise PlanningError(f"Cannot set a label on {s[1]}: not a node")


# ---- the pattern graph ---------------------------------------------------------------------------------------
class PatternGraph:
    """SingleTableGraph: one table whose entity variables are the graph's entities."""

    def __init__(self, backend, table, header: List[str], node_vars: Sequence[str], rel_vars: Sequence[str], tags):
        self.backend = backend
        self.table = table
        self.header = list(header)
        self.node_vars = list(node_vars)
        self.rel_vars = list(rel_vars)
        self.tags = frozenset(tags)
        self._entity_tables = None

    def has_pattern(self) -> bool:
        return True

    # -- what a variable owns
    def _labels(self, v: str) -> List[str]:
        return sorted(h[len(v) + 1:] for h in self.header if h.startswith(v + ":"))

    def _props(self, v: str) -> Dict[str, int]:
        types = self.table.columnType
        return {h[len(v) + 1:]: types[h] for h in self.header if h.startswith(v + ".") and not h.startswith(v + ".__")}

    def _merged_props(self, per_var: Sequence[Dict[str, int]]) -> Dict[str, int]:
        props: Dict[str, int] = {}
        for p in per_var:
            for k, ty in p.items():
                if k in props and props[k] != ty:
                    raise _planner().PlanningError(f"property '{k}' has conflicting types across the pattern graph's variables")
                props[k] = ty
        return props

    def _empty(self, schema):
        return self.backend.table([_planner().ColumnData(n, ty, np.zeros(0, dtype=np.float64 if ty == F64 else np.int64))
                                   for n, ty in schema])

    # -- scans (SingleTableGraph.scala:67-106): per variable select, filter, distinct; aligned; unionAll, no
    #    distinct across the variables
    def node_scan(self, var: str, labels: Sequence[str]):
        req = list(labels)
        sel = [v for v in self.node_vars if set(req) <= set(self._labels(v))]
        all_labels = sorted(set(req).union(*[self._labels(v) for v in sel]))
        props = self._merged_props([self._props(v) for v in sel])
        header = [var] + [f"{var}:{l}" for l in all_labels] + [f"{var}.{k}" for k in sorted(props)]
        if not sel:
            return self._empty([(var, I64)] + [(f"{var}:{l}", BOOL) for l in all_labels]), header
        ops = []
        for v in sel:
            cols = owned(self.header, v)
            pred = ands(IsNotNull(Col(v)), *[BinOp("=", Col(f"{v}:{l}"), Lit(True)) for l in req])
            t = self.table.select(*cols).filter(pred).distinct(*cols)
            have_l, have_p = set(self._labels(v)), self._props(v)
            out = [(Col(v), var)]
            out += [(Col(f"{v}:{l}") if l in have_l else Lit(False), f"{var}:{l}") for l in all_labels]
            out += [(Col(f"{v}.{k}") if k in have_p else Lit(None, props[k]), f"{var}.{k}") for k in sorted(props)]
            ops.append(_aligned(t, out, header))
        res = ops[0]
        for o in ops[1:]:
            res = res.unionAll(o)
        return res, header

    def rel_scan(self, var: str, types: Sequence[str]):
        sel = list(self.rel_vars)
        props = self._merged_props([self._props(v) for v in sel])
        header = [var, f"{var}.__src", f"{var}.__dst", f"{var}.__type"] + [f"{var}.{k}" for k in sorted(props)]
        if not sel:
            return self._empty([(var, I64), (f"{var}.__src", I64), (f"{var}.__dst", I64), (f"{var}.__type", STR)]), header
        ops = []
        for v in sel:
            cols = owned(self.header, v)
            conj = [IsNotNull(Col(c)) for c in _id_cols(v, True)]
            if types:
                conj.append(In(Col(f"{v}.__type"), tuple(Lit(t) for t in types)))
            t = self.table.select(*cols).filter(ands(*conj)).distinct(*cols)
            have_p = self._props(v)
            out = [(Col(v), var), (Col(f"{v}.__src"), f"{var}.__src"), (Col(f"{v}.__dst"), f"{var}.__dst"),
                   (Col(f"{v}.__type"), f"{var}.__type")]
            out += [(Col(f"{v}.{k}") if k in have_p else Lit(None, props[k]), f"{var}.{k}") for k in sorted(props)]
            ops.append(_aligned(t, out, header))
        res = ops[0]
        for o in ops[1:]:
            res = res.unionAll(o)
        return res, header

    # -- entity tables: one per variable and per label combination (or type) its rows hold
    def entity_tables(self):
        """(node tables, relationship tables) as planner.EntityTable: the combinations are read from a ``group`` over
        the flag columns (the type column), together with each property's count of values -- a property column that is
        null in every row of a combination's table is no key of it."""
        if self._entity_tables is not None:
            return self._entity_tables
        pl = _planner()
        dictionary = self.backend.dictionary
        nodes, rels = [], []
        for v in self.node_vars:
            cols = owned(self.header, v)
            labels, props = self._labels(v), self._props(v)
            flags = [f"{v}:{l}" for l in labels]
            # a NULL flag (the entity of an OPTIONAL MATCH miss, a copy of one) is not set
            norm = [(Coalesce((Col(f), Lit(False))), f) for f in flags]
            t = self.table.select(*cols).filter(IsNotNull(Col(v))).distinct(*cols)
            if norm:
                t = t.withColumns(*norm)
            if t.size == 0:  # an action of its own: the distinct runs once, the group and the filters read its rows
                continue
            counts = [("count", f"{v}.{k}", False, f"__n_{i}") for i, k in enumerate(sorted(props))]
            groups = t.group(flags, counts + [("count_star", None, False, "__rows")])
            for row in _host_rows(groups, dictionary):
                if not row["__rows"]:  # the global aggregate of an empty table
                    continue
                combo = frozenset(l for l, f in zip(labels, flags) if row[f])
                keys = {k: props[k] for i, k in enumerate(sorted(props)) if row[f"__n_{i}"] > 0}
                pred = ands(*[Col(f) if l in combo else Not(Col(f)) for l, f in zip(labels, flags)])
                part = t if (isinstance(pred, Lit) and pred.value is True) else t.filter(pred)
                out = [(Col(v), pl.ID)] + [(Col(f"{v}.{k}"), k) for k in sorted(keys)]
                tab = _aligned(part, out, [pl.ID] + sorted(keys))
                nodes.append(pl.EntityTable("node", combo, keys, tab))
        for v in self.rel_vars:
            cols = owned(self.header, v)
            props = self._props(v)
            t = self.table.select(*cols).filter(ands(*[IsNotNull(Col(c)) for c in _id_cols(v, True) + [f"{v}.__type"]]))
            t = t.distinct(*cols)
            if t.size == 0:  # as above: materialised once
                continue
            counts = [("count", f"{v}.{k}", False, f"__n_{i}") for i, k in enumerate(sorted(props))]
            groups = t.group([f"{v}.__type"], counts + [("count_star", None, False, "__rows")])
            for row in _host_rows(groups, dictionary):
                ty = row[f"{v}.__type"]
                keys = {k: props[k] for i, k in enumerate(sorted(props)) if row[f"__n_{i}"] > 0}
                part = t.filter(BinOp("=", Col(f"{v}.__type"), Lit(ty)))
                out = [(Col(v), pl.ID), (Col(f"{v}.__src"), pl.SRC), (Col(f"{v}.__dst"), pl.DST)]
                out += [(Col(f"{v}.{k}"), k) for k in sorted(keys)]
                tab = _aligned(part, out, [pl.ID, pl.SRC, pl.DST] + sorted(keys))
                rels.append(pl.EntityTable("rel", frozenset([ty]), keys, tab))
        self._entity_tables = (nodes, rels)
        return self._entity_tables

    def to_scan_graph(self):
        return to_scan_graph(self)


def _aligned(t, cols: Sequence[Tuple[Expr, str]], header: Sequence[str]):
    """alignWith: the columns renamed (through temporaries: a target name may be a source name) and put in order."""
    tmp = [f"__al{i}" for i in range(len(cols))]
    t = t.withColumns(*[(e, n) for (e, _), n in zip(cols, tmp)]).select(*tmp)
    return t.withColumns(*[(Col(n), name) for (_, name), n in zip(cols, tmp)]).select(*header)


def _host_rows(table, dictionary) -> List[dict]:
    pl = _planner()
    cols = table.to_columns()
    out = []
    for r in range(table.size):
        row = {}
        for c in cols:
            ok = c.valid is None or bool(c.valid[r])
            row[c.name] = pl.decode_value(c.type, c.values[r], dictionary) if ok else None
        out.append(row)
    return out


def _stored_columns(table):
    """The table's columns as a stored table holds them: a computed column is nullable by type, a key column of an
    entity table is not, so a validity mask that excludes no row is dropped."""
    pl = _planner()
    return [pl.ColumnData(c.name, c.type, c.values, None if c.valid is None or np.asarray(c.valid, dtype=bool).all() else c.valid)
            for c in table.to_columns()]


def _one_table_per_combination(tables):
    """One entity table per label combination (per type), as CAPSScanGraphFactory lays a graph out: the tables of a
    combination -- one per variable of a pattern graph, one per member of a union -- aligned, union'ed and made
    distinct, which is the union graph's Distinct on the scanned entity."""
    pl = _planner()
    by: Dict[object, list] = {}
    for e in tables:
        by.setdefault(e.labels, []).append(e)
    out = []
    for labels, es in by.items():
        props: Dict[str, int] = {}
        for e in es:
            for k, ty in e.props.items():
                if k in props and props[k] != ty:
                    raise pl.PlanningError(f"property '{k}' has conflicting types across the tables of {sorted(labels)}")
                props[k] = ty
        is_rel = es[0].kind == "rel"
        header = [pl.ID] + ([pl.SRC, pl.DST] if is_rel else []) + sorted(props)
        parts = []
        for e in es:
            cols = [(Col(e.id_col), pl.ID)] + ([(Col(e.src_col), pl.SRC), (Col(e.dst_col), pl.DST)] if is_rel else [])
            cols += [(Col(k) if k in e.props else Lit(None, props[k]), k) for k in sorted(props)]
            parts.append(_aligned(e.table, cols, header))
        t = parts[0]
        for q in parts[1:]:
            t = t.unionAll(q)
        out.append(pl.EntityTable(es[0].kind, labels, props, t.distinct(*header)))
    return out


def to_scan_graph(graph):
    """The CachedDataSource analogue: ``graph``'s entity tables (a PatternGraph's, a UnionGraph's) materialised,
    registered as entity tables and compacted where their ids are sparse -- tagged ids are -- so that queries over the
    stored graph take the fused routes like any ScanGraph."""
    pl = _planner()
    backend = graph.backend
    gn, gr = graph.entity_tables()
    gn, gr = _one_table_per_combination(gn), _one_table_per_combination(gr)
    nodes, rels = [], []
    for e in gn:
        tab = backend.table(_stored_columns(e.table)).as_node_table(e.id_col)
        nodes.append(pl.EntityTable("node", e.labels, e.props, tab, e.id_col))
    for e in gr:
        tab = backend.table(_stored_columns(e.table)).as_rel_table(e.id_col, e.src_col, e.dst_col)
        rels.append(pl.EntityTable("rel", e.labels, e.props, tab, e.id_col, e.src_col, e.dst_col))
    backend.compact_if_sparse([e.table for e in nodes], [e.table for e in rels])
    return pl.ScanGraph(backend, nodes, rels, graph.tags)


# ---- planConstructGraph ------------------------------------------------------------------------------------
def plan_construct(backend, table, header: Sequence[str], node_vars: Set[str], rel_vars: Sequence[str],
                   graph_of: Mapping[str, object], spec: dict, catalog: Mapping[object, object]):
    """ConstructGraphPlanner.planConstructGraph over the bindings ``table``.  ``graph_of`` names the graph each entity
    variable was matched from (the ``cypherType.graph`` the reference reads); ``catalog`` resolves names.  Returns
    (constructed graph, PatternGraph, constructTagStrategy)."""
    pl = _planner()
    validate(spec, set(node_vars), set(rel_vars))
    on = list(spec.get("on", []))
    for g in on:
        if g not in catalog:
            raise pl.PlanningError(f"unknown graph {g} in CONSTRUCT ON")
    clones = [tuple(c) for c in spec.get("clones", [])]
    creates = list(spec.get("creates", []))
    sets = list(spec.get("sets", []))
    header = list(header)
    is_rel = {v: True for v in rel_vars}
    is_rel.update({v: False for v in node_vars})

    # the tag strategy: the ON plan's retaggings fixed, the match graphs fitted in after them (:55-76)
    match_graphs = []
    for _, orig in clones:
        g = graph_of[orig]
        if g not in [k for k, _ in match_graphs]:
            match_graphs.append((g, catalog[g].tags))
    on_strategy, strategy = tag_strategy([(g, catalog[g].tags) for g in on], match_graphs)

    # aliases of CLONE, then the clones' ids retagged (:78-91)
    alias_cols = []
    for alias, orig in clones:
        if alias != orig:
            if alias in is_rel:
                raise pl.PlanningError(f"CLONE {orig} AS {alias}: {alias} is already bound")
            for h in owned(header, orig):
                alias_cols.append((Col(h), alias + h[len(orig):]))
            is_rel[alias] = is_rel[orig]
    if alias_cols:
        table = table.withColumns(*alias_cols)
        header += [n for _, n in alias_cols]
    retag = []
    for alias, orig in clones:
        rep = strategy[graph_of[orig]]
        if any(f != t for f, t in rep.items()):  # an identity replacement is the reference's no-op CaseExpr
            retag += [(expr_replace_tags(Col(c), rep), c) for c in _id_cols(alias, is_rel[alias])]
    if retag:
        table = table.withColumns(*retag)

    # created entities: nodes before relationships, as relationships copy their endpoints' ids (:93-181)
    created_tags: Set[int] = set()
    new_nodes = [c for c in creates if "node" in c and c["node"] not in is_rel]
    new_rels = [c for c in creates if "rel" in c and c["rel"] not in is_rel]
    if creates:
        tag = pick_free_tag({t for m in strategy.values() for t in m.values()})
        created_tags = {tag}
        cols: Dict[str, Expr] = {}
        for k, c in enumerate(new_nodes):
            v, base = c["node"], c.get("copy_of")
            for l in c.get("labels", []):
                cols[f"{v}:{l}"] = Lit(True)
            if base is not None:  # copied labels, then copied properties, win over created ones (Map ++)
                for h in owned(header, base):
                    if h != base:
                        cols[v + h[len(base):]] = Col(h)
            cols[v] = _created_id(generate_id(k, len(new_nodes)), tag, base)
            is_rel[v] = False
        if cols:
            table = table.withColumns(*[(e, n) for n, e in cols.items()])
            header += [n for n in cols if n not in header]
        cols = {}
        for k, c in enumerate(new_rels):
            v, base = c["rel"], c.get("copy_of")
            if base is not None:
                for h in owned(header, base):
                    if h not in _id_cols(base, True) and h != f"{base}.__type":
                        cols[v + h[len(base):]] = Col(h)
            cols[f"{v}.__type"] = Lit(c["type"]) if c.get("type") is not None else Col(f"{base}.__type")
            cols[v] = _created_id(generate_id(k, len(new_rels)), tag, base)
            cols[f"{v}.__src"] = Col(c["src"])
            cols[f"{v}.__dst"] = Col(c["dst"])
            is_rel[v] = True
        if cols:
            table = table.withColumns(*[(e, n) for n, e in cols.items()])
            header += [n for n in cols if n not in header]
        # SET items last, replacing a column even with one of another type (addInto); the reference applies them
        # only beside created entities (:101-112), restated as it is
        set_cols = []
        for s in sets:
            if s[0] == "prop":
                set_cols.append((pl.to_expr(s[3], header), f"{s[1]}.{s[2]}"))
            else:
                set_cols += [(Lit(True), f"{s[1]}:{l}") for l in s[2]]
        if set_cols:
            table = table.withColumns(*set_cols)
            header += [n for _, n in set_cols if n not in header]

    # every variable of the input goes, except the clones kept under their own names (:116-121)
    aliased_originals = {orig for alias, orig in clones if alias != orig}
    keep = {alias for alias, _ in clones} - aliased_originals
    keep |= {c["node"] for c in new_nodes} | {c["rel"] for c in new_rels}
    out_header = [h for h in header if any(h in owned(header, v) for v in keep)]
    node_out = [v for v in is_rel if v in keep and not is_rel[v]]
    rel_out = [v for v in is_rel if v in keep and is_rel[v]]
    if out_header:
        table = table.select(*out_header)
    else:  # nothing kept: no entity, whatever the bindings were
        table = table.select(header[0]).limit(0)
        out_header = []

    tags_used = set(created_tags)
    for g, rep in strategy.items():
        tags_used |= {rep[t] for t in catalog[g].tags}
    pattern = PatternGraph(backend, table, out_header, node_out, rel_out, tags_used)
    members = [(pattern, {t: t for t in sorted(pattern.tags)})]
    if len(on) == 1:  # Start(one, its retaggings): no union below the union (:58-59)
        members.insert(0, (catalog[on[0]], on_strategy[on[0]]))
    elif on:
        on_graph = pl.UnionGraph(backend, [(catalog[g], on_strategy[g]) for g in on])
        members.insert(0, (on_graph, {t: t for t in sorted(on_graph.tags)}))
    return pl.UnionGraph(backend, members), pattern, strategy


def _created_id(generated: Expr, tag: int, base) -> Expr:
    """The tagged id of a created entity.  A copy of a base that is NULL in the row (an OPTIONAL MATCH miss) is no
    entity: its id is NULL, which the scans drop.  The row index still counts the row."""
    e = expr_set_tag(generated, tag)
    return e if base is None else Case(((IsNotNull(Col(base)), e),), Lit(None, I64))
