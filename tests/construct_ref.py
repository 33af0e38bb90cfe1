"""CONSTRUCT restated in pure Python over PropertyGraph and binding rows: bindings in, PropertyGraph out.

An independent reading of ConstructGraphPlanner.scala:52-272 and SingleTableGraph.scala:49-106 (no table algebra, none
of capsmi.construct or capsmi.tagging): the same tag strategy (TagSupport.computeRetaggings with the ON plan's
retaggings fixed, ON graphs first), the same id formula (row index + (k << (33 - (floor(ln n) + 1))), tagged), clones
retagged, COPY OF, SET applied last, the pattern graph's entities extracted per variable and made distinct, and the
union with the ON graphs made distinct on the whole entity.

The row index of a binding is its position in the list given; a table may hold the rows in another order, so created
ids compare as sets and up to a bijection (``canonical``).  ``run_case`` drives a golden case of
tests/golden/construct.json with a small matcher for the MATCH patterns those cases use.
"""
import math
from collections import Counter

from capsmi.planner import PGNode, PGRel, PropertyGraph, _Names, parse_pattern

ID_BITS = 54
ID_MASK = (1 << ID_BITS) - 1


# ---- tags and ids ---------------------------------------------------------------------------------------
def set_tag(i, tag):
    return (i & ID_MASK) | (tag << ID_BITS)


def get_tag(i):
    return (i & ((1 << 64) - 1)) >> ID_BITS


def retag(i, rep):
    return set_tag(i, rep[get_tag(i)]) if get_tag(i) in rep else i


def id_offset(k, n):
    return k << (33 - (int(math.floor(math.log(n))) + 1))


def _replacements_for(used, tags):
    if not used:
        return {t: t for t in sorted(tags)}
    if not tags:
        return {t: t for t in sorted(used)}
    nxt = max(max(used), max(tags)) + 1
    out = {}
    for t in sorted(tags):
        if t in used:
            out[t] = nxt
            nxt += 1
    for t in sorted(tags):
        out.setdefault(t, t)
    return out


def _retaggings(graphs, fixed):
    result = {k: dict(v) for k, v in fixed.items()}
    used = {t for v in fixed.values() for t in v.values()}
    for k, tags in graphs:
        if k in result:
            continue
        rep = _replacements_for(used, set(tags)) if (used or tags) else {}
        used |= {rep.get(t, t) for t in tags}
        result[k] = rep
    return result


def tag_strategy(on, match):
    """(ON plan's strategy, construct strategy) for [(graph key, tags)] lists."""
    on_strategy = _retaggings(list(on), {})
    return on_strategy, _retaggings(list(on) + list(match), on_strategy)


def pick_free_tag(used):
    used = set(used)
    if not used:
        return 0
    if max(used) < 1023:
        return max(used) + 1
    return min(set(range(1024)) - used)


# ---- graphs -------------------------------------------------------------------------------------------------
class RefGraph:
    def __init__(self, pg, tags=(0,)):
        self.pg = pg
        self.tags = frozenset(tags)


def _distinct_entities(nodes, rels):
    seen, on, orr = set(), [], []
    for n in nodes:
        key = (n.id, n.labels, tuple(sorted((k, repr(v)) for k, v in n.props.items() if v is not None)))
        if key not in seen:
            seen.add(key)
            on.append(n)
    for r in rels:
        key = (r.id, r.src, r.dst, r.type, tuple(sorted((k, repr(v)) for k, v in r.props.items() if v is not None)))
        if key not in seen:
            seen.add(key)
            orr.append(r)
    return on, orr


def _retagged(pg, rep):
    return ([PGNode(retag(n.id, rep), n.labels, dict(n.props)) for n in pg.nodes],
            [PGRel(retag(r.id, rep), retag(r.src, rep), retag(r.dst, rep), r.type, dict(r.props)) for r in pg.rels])


def _eval(spec, row):
    op = spec[0]
    if op == "lit":
        return spec[1]
    if op == "prop":
        e = row.get(spec[1])
        return None if e is None else e.props.get(spec[2])
    if op in ("var", "id"):
        e = row.get(spec[1])
        return e.id if isinstance(e, (PGNode, PGRel)) else e
    raise NotImplementedError(f"expression {spec!r} in a SET item of the restatement")


def construct(bindings, kinds, graph_of, spec, catalog):
    """bindings: rows {var: PGNode | PGRel | value | None}; kinds: var -> "node" | "rel" for the entity variables;
    graph_of: var -> catalog key.  Returns (RefGraph, the construct tag strategy, the created tag or None)."""
    on = list(spec.get("on", []))
    clones = [tuple(c) for c in spec.get("clones", [])]
    creates = list(spec.get("creates", []))
    match = []
    for _, orig in clones:
        if graph_of[orig] not in [k for k, _ in match]:
            match.append((graph_of[orig], catalog[graph_of[orig]].tags))
    on_strategy, strategy = tag_strategy([(g, catalog[g].tags) for g in on], match)
    kinds = dict(kinds)
    rows = [dict(b) for b in bindings]
    for alias, orig in clones:  # aliases, then the clones retagged
        for row in rows:
            e, rep = row.get(orig), strategy[graph_of[orig]]
            if e is None:
                row[alias] = None
            elif kinds[orig] == "node":
                row[alias] = PGNode(retag(e.id, rep), e.labels, dict(e.props))
            else:
                row[alias] = PGRel(retag(e.id, rep), retag(e.src, rep), retag(e.dst, rep), e.type, dict(e.props))
        kinds[alias] = kinds[orig]
    created_tag = None
    new_nodes = [c for c in creates if "node" in c and c["node"] not in kinds]
    new_rels = [c for c in creates if "rel" in c and c["rel"] not in kinds]
    if creates:
        created_tag = pick_free_tag({t for m in strategy.values() for t in m.values()})
        for k, c in enumerate(new_nodes):
            for r, row in enumerate(rows):
                labels, props, base = set(c.get("labels", [])), {}, c.get("copy_of")
                flags = {l: True for l in labels}
                if base is not None:  # the copied flag columns win, NULL flags of a missing base included
                    b = row.get(base)
                    known = _labels_known(bindings, base)
                    flags.update({l: (None if b is None else l in b.labels) for l in known})
                    props = {} if b is None else dict(b.props)
                if base is not None and row.get(base) is None:  # a copy of an OPTIONAL MATCH miss is no entity
                    row[c["node"]] = None
                    continue
                row[c["node"]] = PGNode(set_tag(r + id_offset(k, len(new_nodes)), created_tag),
                                        frozenset(l for l, v in flags.items() if v), props)
            kinds[c["node"]] = "node"
        for k, c in enumerate(new_rels):
            for r, row in enumerate(rows):
                base = row.get(c["copy_of"]) if c.get("copy_of") is not None else None
                if c.get("copy_of") is not None and base is None:
                    row[c["rel"]] = None
                    continue
                ty = c["type"] if c.get("type") is not None else (None if base is None else base.type)
                s, d = row.get(c["src"]), row.get(c["dst"])
                row[c["rel"]] = PGRel(set_tag(r + id_offset(k, len(new_rels)), created_tag), None if s is None else s.id,
                                      None if d is None else d.id, ty, {} if base is None else dict(base.props))
            kinds[c["rel"]] = "rel"
        for s in spec.get("sets", []):  # SET last; only beside created entities, as the reference has it
            for row in rows:
                e = row.get(s[1])
                if e is None:
                    continue
                if s[0] == "prop":
                    e.props[s[2]] = _eval(s[3], row)
                else:
                    row[s[1]] = PGNode(e.id, frozenset(e.labels | set(s[2])), e.props)
    aliased = {orig for alias, orig in clones if alias != orig}
    keep = ({alias for alias, _ in clones} - aliased) | {c["node"] for c in new_nodes} | {c["rel"] for c in new_rels}
    nodes, rels = [], []
    for v in sorted(keep):  # the pattern graph's scans: per variable, valid entities, distinct
        ents = [row[v] for row in rows if row.get(v) is not None]
        if kinds[v] == "node":
            vn, _ = _distinct_entities(ents, [])
            nodes += vn
        else:
            _, vr = _distinct_entities([], [e for e in ents if e.src is not None and e.dst is not None and e.type is not None])
            rels += vr
    tags = set() if created_tag is None else {created_tag}
    for g, rep in strategy.items():
        tags |= {rep[t] for t in catalog[g].tags}
    if on:  # the union with the ON graphs
        on_nodes, on_rels = [], []
        for g in on:
            gn, gr = _retagged(catalog[g].pg, on_strategy[g])
            on_nodes += gn
            on_rels += gr
        nodes, rels = on_nodes + nodes, on_rels + rels
    nodes, rels = _distinct_entities(nodes, rels)  # UnionGraph's Distinct on the scanned entity, of one member too
    return RefGraph(PropertyGraph(nodes, rels), tags), strategy, created_tag


def _labels_known(bindings, base):
    """The label columns the base variable has in the bindings' header: every label some binding of it carries."""
    out = set()
    for b in bindings:
        if b.get(base) is not None:
            out |= set(b[base].labels)
    return out


# ---- a matcher for the golden cases' patterns -----------------------------------------------------------------
def match(pg, pattern, rows=None, names=None):
    """Bindings of a MATCH pattern (nodes with labels, single relationships with types and a direction, relationship
    uniqueness within the clause) on top of ``rows``."""
    paths = parse_pattern(pattern, names or _Names())
    rows = [dict(r) for r in (rows if rows is not None else [{}])]
    kinds = {}
    clause_rels = []
    for path in paths:
        first = path[0]
        kinds[first.var] = "node"
        rows = [dict(r, **{first.var: n}) if first.var not in r else r for r in rows for n in
                ([x for x in pg.nodes if set(first.labels) <= x.labels] if first.var not in r else
                 ([r[first.var]] if set(first.labels) <= r[first.var].labels else []))]
        for k in range(1, len(path), 2):
            rel, left, right = path[k], path[k - 1], path[k + 1]
            kinds[rel.var], kinds[right.var] = "rel", "node"
            by_id = {n.id: n for n in pg.nodes}
            out = []
            for r in rows:
                for e in pg.rels:
                    if rel.types and e.type not in rel.types:
                        continue
                    if any(r.get(o) is e for o in clause_rels):
                        continue
                    for a, b in (((e.src, e.dst),) if rel.direction == "out" else ((e.dst, e.src),) if rel.direction == "in"
                                 else ((e.src, e.dst), (e.dst, e.src))[: 1 if e.src == e.dst else 2]):
                        if a != r[left.var].id or b not in by_id or not set(right.labels) <= by_id[b].labels:
                            continue
                        if right.var in r and r[right.var].id != b:
                            continue
                        out.append(dict(r, **{rel.var: e, right.var: by_id[b]}))
            rows = out
            clause_rels.append(rel.var)
    return rows, kinds


def _graph_of_text(text):
    from oracle.create_graph import create_graph
    g = create_graph(text) if text else {"nodes": [], "rels": []}
    return PropertyGraph([PGNode(n["id"], frozenset(n["labels"]), dict(n["props"])) for n in g["nodes"]],
                         [PGRel(r["id"], r["src"], r["dst"], r["type"], dict(r["props"])) for r in g["rels"]])


def case_graphs(case):
    """{name: PropertyGraph} of a golden case, the ambient graph under ``case["ambient"]`` (None: the empty graph)."""
    return {name: _graph_of_text(text) for name, text in case["graphs"].items()}


def run_case(case):
    """The case's query over the restatement: {"tags", "nodes", "rels"} of the graph it returns, or {"rows"}."""
    catalog = {name: RefGraph(pg) for name, pg in case_graphs(case).items()}
    catalog.setdefault("session.ambient", RefGraph(PropertyGraph([], [])))
    cur_name = case.get("ambient") or "session.ambient"
    if isinstance(cur_name, list):  # graph.unionAll(graph, ...): the members retagged against each other
        members = [(g, catalog[g].tags) for g in cur_name]
        reps = _retaggings(members, {})
        nodes, rels = [], []
        for g, _ in members:
            gn, gr = _retagged(catalog[g].pg, reps[g])
            nodes += gn
            rels += gr
        nodes, rels = _distinct_entities(nodes, rels)
        cur_name = "session.ambient"
        catalog[cur_name] = RefGraph(PropertyGraph(nodes, rels), {t for r in reps.values() for t in r.values()})
    names, rows, kinds, graph_of, made = _Names(), None, {}, {}, 0
    strategies = []
    q = case["query"]
    for clause in q["clauses"]:
        if "from_graph" in clause:
            cur_name = clause["from_graph"]
        elif "match" in clause:
            rows, k2 = match(catalog[cur_name].pg, clause["match"], rows, names)
            if clause.get("where") is not None:
                rows = [r for r in rows if _where(clause["where"], r)]
            kinds.update(k2)
            for v in k2:
                graph_of.setdefault(v, cur_name)
        elif "unwind" in clause:
            rows = [dict(r, **{clause["as"]: v}) for r in (rows if rows is not None else [{}]) for v in clause["unwind"][1]]
        elif "with" in clause:  # WITH [DISTINCT] entity items
            keep = [spec[1] for _, spec in clause["with"]["items"]]
            rows = [{v: r[v] for v in keep} for r in rows]
            if clause["with"].get("distinct"):
                seen, out = set(), []
                for r in rows:
                    key = tuple(r[v].id for v in keep)
                    if key not in seen:
                        seen.add(key)
                        out.append(r)
                rows = out
            kinds = {v: kinds[v] for v in keep}
        elif "construct" in clause:
            g, strategy, _ = construct(rows if rows is not None else [{}], kinds, graph_of, clause["construct"], catalog)
            strategies.append({str(k): v for k, v in strategy.items()})
            made += 1
            cur_name = f"_constructed{made}"
            catalog[cur_name] = g
            rows, kinds, graph_of = None, {}, {}
    g = catalog[cur_name]
    if q["return"] == "graph":
        return {"tags": sorted(g.tags), "nodes": g.pg.nodes, "rels": g.pg.rels, "strategies": strategies}
    out = []
    for r in rows:
        out.append({alias: _item(spec, r) for alias, spec in q["return"]["items"]})
    return {"rows": out, "strategies": strategies}


def _where(spec, row):
    if spec[0] == "and":
        return all(_where(s, row) for s in spec[1:])
    if spec[0] == "=":
        return _eval(spec[1], row) == _eval(spec[2], row)
    raise NotImplementedError(spec)


def _item(spec, row):
    if spec[0] == "labels":
        return sorted(row[spec[1]].labels)
    if spec[0] == "entity":
        e = row[spec[1]]
        return {"id": e.id, "labels": sorted(e.labels), "props": {k: v for k, v in e.props.items() if v is not None}}
    return _eval(spec, row)


# ---- comparison -----------------------------------------------------------------------------------------------
def _props(p):
    return tuple(sorted((k, repr(v)) for k, v in p.items() if v is not None))


def canonical(nodes, rels, created_tags=()):
    """A graph up to a bijection of the created ids that keeps the tag, applied to node ids and endpoints alike: a
    node is (tag, its id unless created, labels, properties), a relationship (tag, its id unless created, type,
    properties, the start node, the end node); an endpoint that names no node keeps its id."""
    created = set(created_tags)

    def nk(n):
        t = get_tag(n.id)
        return (t, None if t in created else n.id, tuple(sorted(n.labels)), _props(n.props))

    by_id = {}
    for n in nodes:
        by_id.setdefault(n.id, nk(n))
    return (Counter(nk(n) for n in nodes),
            Counter((get_tag(r.id), None if get_tag(r.id) in created else r.id, r.type, _props(r.props),
                     by_id.get(r.src, ("dangling", r.src)), by_id.get(r.dst, ("dangling", r.dst))) for r in rels))


def assert_graph(got, expected):
    """``got`` (run_case's answer, or the device's in the same form) against a case's ``expected``: the rows as a bag;
    or tags, the node and relationship bags by labels / type and properties, the ids where the reference pins them, and
    the schema (label combinations, types, property keys per combination) where the reference states one."""
    if "rows" in expected:
        want = Counter(repr(sorted(r.items())) for r in expected["rows"])
        have = Counter(repr(sorted(r.items())) for r in got["rows"])
        assert have == want, (have, want)
        return
    if "tags" in expected:
        assert sorted(got["tags"]) == expected["tags"], got["tags"]
    nodes, rels = got["nodes"], got["rels"]
    by_id = {n.id: n for n in nodes}

    def node_key(n, with_id):
        return (n.id if with_id else None, tuple(sorted(n.labels)), _props(n.props))

    want_nodes = Counter(((None if "id" not in e else set_tag(e["id"], e.get("tag", 0))), tuple(sorted(e["labels"])),
                          _props(e.get("props", {}))) for e in expected["nodes"])
    ids_pinned = all("id" in e for e in expected["nodes"])
    assert Counter(node_key(n, ids_pinned) for n in nodes) == want_nodes, [node_key(n, ids_pinned) for n in nodes]
    assert len(by_id) == len(nodes), "node ids are not unique"
    want_rels, have_rels = Counter(), Counter()
    rel_ids = all("id" in e for e in expected["rels"])
    for e in expected["rels"]:
        want_rels[(set_tag(e["id"], e.get("tag", 0)) if rel_ids else None, e["type"], _props(e.get("props", {})),
                   tuple(sorted(e["src"]["labels"])), _props(e["src"].get("props", {})),
                   tuple(sorted(e["dst"]["labels"])), _props(e["dst"].get("props", {})))] += 1
    for r in rels:
        assert r.src in by_id and r.dst in by_id, f"relationship {r.id}: an endpoint names no node"
        s, d = by_id[r.src], by_id[r.dst]
        have_rels[(r.id if rel_ids else None, r.type, _props(r.props), tuple(sorted(s.labels)), _props(s.props),
                   tuple(sorted(d.labels)), _props(d.props))] += 1
    assert have_rels == want_rels, (have_rels, want_rels)
    assert len({r.id for r in rels}) == len(rels), "relationship ids are not unique"
    for pin in expected.get("rel_pins", []):  # {"tag", "src_id"?, "src_tag"?, "dst_tag"?}: holds for every relationship
        for r in rels:
            assert get_tag(r.id) == pin["tag"], r
            if "src_id" in pin:
                assert r.src == pin["src_id"], r
            if "dst_tag" in pin:
                assert get_tag(r.dst) == pin["dst_tag"], r
    if "schema" in expected:
        combos = {}
        for n in nodes:
            combos.setdefault(tuple(sorted(n.labels)), set()).update(k for k, v in n.props.items() if v is not None)
        types = {}
        for r in rels:
            types.setdefault(r.type, set()).update(k for k, v in r.props.items() if v is not None)
        want = expected["schema"]
        assert {",".join(c): sorted(k) for c, k in combos.items()} == want["nodes"], combos
        assert {t: sorted(k) for t, k in types.items()} == want["rels"], types
