"""The integer tables that the kernels cannot validate, prepared on the host in pure torch (no library, no GPU): one integer
check, one range check, one ``incidence`` builder, the degree-sorted packing order of the MAF layers (``stable_order``,
``packed_rows``) and one ``Cache`` class, then the index tables of ``internal_coordinates``, the level-sorted Z-matrix of
``zmatrix_place`` and the node-incidence list of ``edge_geometry_backward`` built on them."""
import collections

import torch


def integer_table(table, name, device='cpu'):
    """``table`` as a detached int64 tensor on ``device``; ValueError for a floating-point, complex or bool one."""
    table = torch.as_tensor(table)
    if table.is_floating_point() or table.is_complex() or table.dtype == torch.bool:
        raise ValueError(f'{name} must hold integer indices, got {table.dtype}')
    return table.detach().to(device, torch.int64)


def out_of_range(table, n):
    """``(min, max)`` of a table with an entry outside ``[0, n)``, else ``None``.  One read-back (one synchronisation)."""
    if table.numel():
        lo, hi = torch.stack([table.min(), table.max()]).tolist()
        if lo < 0 or hi >= n:
            return lo, hi


def check_range(table, name, n):
    bad = out_of_range(table, n)
    if bad:
        raise ValueError(f'{name} has an index outside [0, {int(n)}): min {bad[0]}, max {bad[1]}')


def incidence(keys, n_bins):
    """The CSR list ``(start (n_bins + 1,), order (n_items,))`` of ``keys`` (n_items,) in ``[0, n_bins)``, int64 on the device
    of ``keys``: ``order[start[b]:start[b + 1]]`` are the positions of ``b`` in ``keys``, ascending (a stable sort)."""
    order = torch.sort(keys, stable=True).indices
    start = torch.zeros(n_bins + 1, dtype=torch.int64, device=keys.device)
    start[1:] = torch.cumsum(torch.bincount(keys, minlength=n_bins), 0)
    return start, order


def stable_order(degrees):
    """``(order, position)`` of a degree vector (torch, numpy or a list) as CPU int64 tensors: ``order[p]`` = the unit at packed
    position ``p`` (stable sort by degree), ``position[u]`` = the packed position (the slot) of unit ``u``.  THE order of every
    degree-sorted packing: hidden units (``MADE.plan``), output rows (``packed_rows``), the float64 blocked inverse."""
    degrees = torch.as_tensor(degrees).detach().to('cpu', torch.int64)
    order = torch.argsort(degrees, stable=True)
    position = torch.empty_like(order)
    position[order] = torch.arange(len(order))
    return order, position


def packed_rows(position, P_real, P, tiling=None):
    """Packed row of every output row ``o = p * n + t`` (parameter ``p < P_real`` of feature ``t`` in slot ``position[t]``) of a
    MADE output layer packed feature-major in slot order, ``P`` parameter rows per slot (``P_real < P``: the others stay
    zero).  No ``tiling``: row ``slot * P + p`` (the backward).  ``tiling = (FT, tile_cols)``: the fused kernels' column tiles
    of ``FT`` x 16 slots, ``[16 slots][parameter][slot]`` inside a tile, relative to the first tile of the group."""
    n = len(position)
    sl = position.repeat(P_real)
    pp = torch.arange(P_real).repeat_interleave(n)
    if tiling is None:
        return sl * P + pp
    FT, tile_cols = tiling
    return (sl // (16 * FT)) * tile_cols + (((sl // 16) % FT) * P + pp) * 16 + sl % 16


class Cache:
    """The last ``size`` results of one family, newest last, under the caller's keys (``None``: never found, never stored) with
    the caller's tensors (``held``: ``get`` can ask for these very objects), whose ``id()`` or data pointer stays theirs."""

    def __init__(self, size):
        self.size, self.entries = size, []                            # entries: (key, the caller's tensors, value)

    def get(self, key, held=None):
        for k, h, value in self.entries:
            if k == key and (held is None or all(a is b for a, b in zip(h, held))):
                return value

    def put(self, key, held, value):
        if key is not None:
            self.entries.append((key, held, value))
            del self.entries[:-self.size]
        return value


def identity_key(tensors, *rest):
    """The key of ``tensors`` (each a tensor or ``None``) by identity, version and shape, after ``rest``; ``None`` if one is
    no tensor (a list, a numpy array) or has no version counter (an inference tensor): a write to it would not show."""
    try:
        return rest + tuple(None if t is None else (id(t), t._version, tuple(t.shape)) for t in tensors)
    except (AttributeError, RuntimeError):
        return None


_INDEX_CACHE, _ZMATRIX_CACHE, _EDGE_CACHE = Cache(size=8), Cache(size=8), Cache(size=4)
TABLE_ROWS = (('pairs', 2), ('triples', 3), ('quads', 4))



def check_index_table(table, name, n_rows, n_atoms):
    """One index table on the host: ``(n_rows, count)`` integers in ``[0, n_atoms)`` as a CPU int64 tensor, else ValueError;
    ``None`` is the empty table."""
    if table is None:
        return torch.empty(n_rows, 0, dtype=torch.int64)
    table = torch.as_tensor(table)
    if table.dim() != 2 or table.shape[0] != n_rows:
        raise ValueError(f'{name} must have shape ({n_rows}, n), got {tuple(table.shape)}')
    table = integer_table(table, name)
    check_range(table, name, n_atoms)
    return table


def build_index_tables(pairs, triples, quads, n_atoms, device):      # (index_tables without its cache)
    host = [check_index_table(t, name, rows_, n_atoms) for t, (name, rows_) in zip((pairs, triples, quads), TABLE_ROWS)]
    counts = [t.shape[1] for t in host]
    if sum(counts) > (2 ** 31 - 1) // 4 or n_atoms > (2 ** 31 - 1) // 4:
        raise ValueError(f'{sum(counts)} table entries of {n_atoms} atoms are too many for int32 items')
    # entry e of a table with slots s: atom table[s, e], item 4 * (offset + e) + s, in table order within an atom
    atoms, items, offset = [], [], 0
    for t in host:
        e = torch.arange(t.shape[1]).unsqueeze(1) + offset
        items.append((4 * e + torch.arange(t.shape[0]).unsqueeze(0)).reshape(-1))
        atoms.append(t.t().reshape(-1))
        offset += t.shape[1]
    start, order = incidence(torch.cat(atoms), n_atoms)
    return tuple(t.to(torch.int32).contiguous().to(device) for t in (*host, start, torch.cat(items)[order]))


def index_tables(pairs, triples, quads, n_atoms, device):
    """The three index tables as the internal-coordinate kernels take them: validated HERE, on the host (ValueError on a
    wrong shape or an index outside ``[0, n_atoms)``; the kernels cannot reject), then ``(pairs, triples, quads,
    atom_start, atom_items)`` as int32 tensors on ``device``.  ``atom_start`` / ``atom_items`` is the incidence list the
    backward kernel sums over: for every atom the entries it appears in, in table order, as ``4 * entry + slot``.
    The last few results are kept, by identity and version of the tensors: a table used step after step is prepared once."""
    given = (pairs, triples, quads)
    key = identity_key(given, int(n_atoms), str(device))
    return _INDEX_CACHE.get(key, given) or _INDEX_CACHE.put(key, given, build_index_tables(*given, n_atoms, device))


ZMATRIX_LDS_LIMIT = 160 * 1024           # bytes of LDS one sample row may take (csrc/zmatrix.hip)
ZMATRIX_MAX_ATOMS = ZMATRIX_LDS_LIMIT // 24          # the forward keeps 3 doubles per atom
ZMATRIX_MAX_PLACED = ZMATRIX_LDS_LIMIT // 72         # the backward keeps 9 doubles per placed atom
ZMatrixTables = collections.namedtuple('ZMatrixTables', 'rows level_start fixed atom_start atom_items')


def check_zmatrix(z_matrix, fixed_atoms, n_atoms):
    """A Z-matrix on the host: ``z_matrix`` ``(n_ic, 4)`` integer rows ``(i, j, k, l)`` -- atom ``i`` is placed from the
    atoms ``j, k, l`` -- in any order, ``fixed_atoms`` ``(n_fixed,)`` the atoms whose positions are given.  Returns both as
    CPU int64 tensors and the level of every row (the fixed atoms are level 0, an atom is one level above the highest of
    its references).  ValueError unless: integer dtypes; the shapes above; every index in ``[0, n_atoms)`` (a negative
    entry, bgflow's ``-1`` of a global row, is not supported); four distinct atoms in a row; no atom placed twice, fixed
    twice, or both; fixed and placed atoms together exactly ``range(n_atoms)``; at least 3 fixed atoms; no cycle; and a
    size the kernels hold in LDS."""
    z, fixed = integer_table(z_matrix, 'z_matrix'), integer_table(fixed_atoms, 'fixed_atoms')
    if z.dim() != 2 or z.shape[1] != 4:
        raise ValueError(f'z_matrix must have shape (n_ic, 4), got {tuple(z.shape)}')
    if fixed.dim() != 1:
        raise ValueError(f'fixed_atoms must have shape (n_fixed,), got {tuple(fixed.shape)}')
    for t, name in ((z, 'z_matrix'), (fixed, 'fixed_atoms')):
        lo, hi = out_of_range(t, n_atoms) or (0, -1)
        if lo < 0:
            raise ValueError(f'{name} has a negative entry ({lo}): rows that place an atom from the global '
                             'frame are not supported, every reference must be an atom')
        if hi >= n_atoms:
            raise ValueError(f'{name} has an index outside [0, {n_atoms}): max {hi}')
    if len(fixed) < 3:
        raise ValueError(f'a Z-matrix needs at least 3 fixed atoms to place the first row from, got {len(fixed)}')
    srt = z.sort(dim=1).values
    if bool((srt[:, 1:] == srt[:, :-1]).any()):
        bad = int((srt[:, 1:] == srt[:, :-1]).any(1).nonzero()[0])
        raise ValueError(f'z_matrix row {bad} {z[bad].tolist()} does not name four distinct atoms')
    placed_count, fixed_count = torch.bincount(z[:, 0], minlength=n_atoms), torch.bincount(fixed, minlength=n_atoms)
    for wrong, how in ((placed_count > 1, 'is placed twice'), (fixed_count > 1, 'is fixed twice'),
                       ((placed_count > 0) & (fixed_count > 0), 'is both fixed and placed'),
                       (placed_count + fixed_count == 0, f'of the {n_atoms} atoms is neither fixed nor placed')):
        if bool(wrong.any()):
            raise ValueError(f'atom {int(wrong.nonzero()[0])} {how}')
    if n_atoms > ZMATRIX_MAX_ATOMS or len(z) > ZMATRIX_MAX_PLACED:
        raise ValueError(f'{n_atoms} atoms, {len(z)} of them placed: the kernels keep a row in {ZMATRIX_LDS_LIMIT} bytes of '
                         f'LDS, which holds at most {ZMATRIX_MAX_ATOMS} atoms and {ZMATRIX_MAX_PLACED} placed atoms')
    # levels: a row is ready once its three references have a level
    atom_level = torch.full((n_atoms,), -1, dtype=torch.int64)
    atom_level[fixed] = 0
    row_level = torch.full((len(z),), -1, dtype=torch.int64)
    while bool((row_level < 0).any()):
        refs = atom_level[z[:, 1:]]
        ready = (row_level < 0) & (refs >= 0).all(1)
        if not bool(ready.any()):
            raise ValueError(f'z_matrix has a cycle: row {int((row_level < 0).nonzero()[0])} can never be placed')
        row_level[ready] = refs[ready].max(1).values + 1
        atom_level[z[ready, 0]] = row_level[ready]
    return z, fixed, row_level


def _zmatrix_prepared(z_matrix, fixed_atoms, n_atoms, device):
    given, n_atoms = (z_matrix, fixed_atoms), int(n_atoms)
    key = identity_key(given, n_atoms, str(device))
    prepared = _ZMATRIX_CACHE.get(key, given)
    if prepared is not None:
        return prepared
    z, fixed, row_level = check_zmatrix(z_matrix, fixed_atoms, n_atoms)
    # rows sorted by level (the placed rows have levels 1, 2, ...), the caller's order kept within a level
    level_start, order = incidence(row_level - 1, int(row_level.max()) if len(z) else 0)
    rows_ = torch.cat([z[order].t(), order.unsqueeze(0)])                   # (5, n_ic): i, j, k, l, column
    # sorted row s names atom rows_[1 + slot, s] as reference `slot`: item 4 * s + slot, in table order within an atom
    start, by_atom = incidence(rows_[1:4].t().reshape(-1), n_atoms)
    items = (4 * torch.arange(len(z)).unsqueeze(1) + torch.arange(3).unsqueeze(0)).reshape(-1)[by_atom]
    place = ZMatrixTables(*(t.to(torch.int32).contiguous().to(device) for t in (rows_, level_start, fixed, start, items)))
    # the same Z-matrix for the way back (internal_coordinates), one entry per row in the caller's order, kept in THIS cache
    index = build_index_tables(z[:, :2].t().contiguous(), z[:, :3].t().contiguous(), z.t().contiguous(), n_atoms, device)
    return _ZMATRIX_CACHE.put(key, given, (place, index, fixed.to(device)))


def zmatrix_tables(z_matrix, fixed_atoms, n_atoms, device):
    """A Z-matrix as the placement kernels take it: validated HERE, on the host (``check_zmatrix``: the kernels cannot
    reject), then ``ZMatrixTables(rows, level_start, fixed, atom_start, atom_items)`` as int32 tensors on ``device``:
    ``rows`` ``(5, n_ic)``: the Z-matrix rows sorted by level (the caller's order within a level) as columns ``(i, j, k,
    l)``, and in the fifth row the permutation back: the caller's row, which is the column of ``(d, a, t)`` with the values
    of that atom.  ``level_start``: ``n_levels + 1`` offsets into the sorted rows.  ``fixed``: the fixed atoms.
    ``atom_start`` / ``atom_items``: the incidence list the backward kernel gathers over, for every atom the rows placed
    from it, in sorted order, as ``4 * sorted row + slot`` (slot 0, 1, 2: the atom is the row's j, k, l).
    The last few results are kept, keyed by the identity, version and shape of the two tensors given."""
    return _zmatrix_prepared(z_matrix, fixed_atoms, n_atoms, device)[0]


def zmatrix_index_tables(z_matrix, fixed_atoms, n_atoms, device):
    """The same Z-matrix for ``internal_coordinates``: ``(index tables, fixed atoms)`` -- the five tensors of
    ``index_tables`` for the pairs ``(i, j)``, triples ``(i, j, k)`` and quads ``(i, j, k, l)`` of the rows in the caller's
    order, and the fixed atoms as an int64 tensor on ``device``.  Validated and cached with ``zmatrix_tables``."""
    return _zmatrix_prepared(z_matrix, fixed_atoms, n_atoms, device)[1:]


def incidence_lists(edges, n_nodes):
    """The node-incidence list (CSR) of a ``(2, E)`` edge list, the host logic of the backward of ``edge_geometry``:
    ``(node_ptr (n_nodes + 1,), incident (2 E,))`` as int64 tensors on the device of ``edges`` (CPU tensors, numpy arrays and
    lists stay on the CPU).  ``incident[node_ptr[n]:node_ptr[n + 1]]`` holds the items ``2 e + role`` of node ``n`` in
    ascending order: role 0 where ``n`` is the source ``edges[0, e]``, role 1 where it is the destination ``edges[1, e]`` --
    ascending edges, the source entry first on a tie (``incidence``).  The indices are taken as given (``check_edges``)."""
    edges = torch.as_tensor(edges)
    if edges.dim() != 2 or edges.shape[0] != 2:
        raise ValueError(f'edges must have shape (2, n_edges), got {tuple(edges.shape)}')
    return incidence(edges.to(torch.int64).t().reshape(-1), int(n_nodes))     # item i = 2 e + role names node edges[role, e]


def edge_entry(edges, n_nodes):
    """The cache entry of a validated ``edges`` tensor: ``[contiguous int64 edges, incidence list or None]``.  Validation
    happens HERE, on the host (ValueError; the kernels never launch with a bad index), once per tensor: the last few are kept,
    keyed by the data pointer, version, layout and device of the tensor: a list used step after step is read back once."""
    if not isinstance(edges, torch.Tensor):
        raise TypeError('edges must be a torch.Tensor')
    if edges.dim() != 2 or edges.shape[0] != 2:
        raise ValueError(f'edges must have shape (2, n_edges), got {tuple(edges.shape)}')
    try:                                                              # (an inference tensor has no version: not cached)
        key = (edges.data_ptr(), edges._version, edges.shape, edges.stride(), edges.dtype, str(edges.device), int(n_nodes))
    except RuntimeError:
        key = None
    entry = _EDGE_CACHE.get(key)
    if entry is None:
        checked = integer_table(edges, 'edges', edges.device) if edges.numel() else edges.detach().to(torch.int64)
        check_range(checked, 'edges', n_nodes)
        entry = _EDGE_CACHE.put(key, edges, [checked.contiguous(), None])
    return entry


def check_edges(edges, n_nodes):
    """``edges`` validated on the host -- shape ``(2, E)``, integers, every index in ``[0, n_nodes)``, else ValueError -- as a
    contiguous int64 tensor on its device (an empty list passes with any dtype).  Cached per tensor."""
    return edge_entry(edges, n_nodes)[0]


def edge_incidence(edges, n_nodes, entry=None):
    """``incidence_lists`` of a validated ``edges`` tensor (or of its ``edge_entry``, where the caller has it) on its device,
    built when first asked for and rebuilt when the tensor changes (its version counts in-place writes)."""
    entry = entry or edge_entry(edges, n_nodes)
    if entry[1] is None:
        entry[1] = incidence_lists(entry[0], n_nodes)
    return entry[1]
