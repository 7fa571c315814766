"""pgl_amd.Graph -- host-side mirror of the reference's `pgl.Graph` message-passing API
(pgl/graph.py), re-expressed over libpglamd's HIP kernels.

Same names, argument meaning and error behaviour as the reference for the hot-path surface:
    send / recv / send_recv / send_u_recv / send_ue_recv / send_uv     (pgl/graph.py:694-966)
    sorted_edges / indegree / outdegree / adj_src_index / adj_dst_index / get_segment_ids
    tensor() / numpy() / dump() / load()
Differences, all deliberate:
  * tensor mode lives on the MI355X (torch-ROCm tensors as the device container); there is no
    CPU tensor mode and no silent fallback -- without a GPU, tensor() raises;
  * send_recv / send_u_recv / send_ue_recv run on the graph's cached dst-sorted CSR with the
    atomic-free flat kernel (K1/K2) instead of a per-edge atomic scatter over raw COO;
  * num_nodes stays a Python int in both modes (the reference turns it into a 1-element tensor).
"""
import json
import os

import numpy as np
import torch

from . import autograd as ag
from . import ops
from . import edge_tensor as _et
from .message import Message
from .utils import op
from .utils.edge_index import EdgeIndex
from .utils.helper import check_is_tensor, maybe_num_nodes, to_device_tensor

_REDUCE = ("sum", "mean", "max", "min")
_MSGOP = ("add", "sub", "mul", "div")


class Graph(object):
    """Graph(edges, num_nodes=None, node_feat=None, edge_feat=None, **kwargs) -- pgl/graph.py:38-193."""

    def __init__(self, edges, num_nodes=None, node_feat=None, edge_feat=None, **kwargs):
        self._node_feat = node_feat if node_feat is not None else {}
        self._edge_feat = edge_feat if edge_feat is not None else {}
        if not check_is_tensor(edges):
            edges = np.asarray(edges, dtype="int64") if not (isinstance(edges, np.ndarray) and edges.dtype == np.int64) else edges
            if edges.size == 0:
                edges = edges.reshape(0, 2)
        self._edges = edges
        if self._edges.ndim != 2 or self._edges.shape[1] != 2:
            raise ValueError("edges must have shape (num_edges, 2)")
        self._num_nodes = int(num_nodes) if num_nodes is not None else maybe_num_nodes(self._edges)
        self._adj_src_index = kwargs.get("adj_src_index", None)
        self._adj_dst_index = kwargs.get("adj_dst_index", None)
        self._is_tensor = check_is_tensor(self._edges, *self._node_feat.values(), *self._edge_feat.values()) or \
            any(ix is not None and ix.is_tensor() for ix in (self._adj_src_index, self._adj_dst_index))
        self._device = None
        if self._is_tensor:
            dev = next((t.device for t in [self._edges, *self._node_feat.values(), *self._edge_feat.values()]
                        if isinstance(t, torch.Tensor)), None)
            self._to_tensor_inplace(dev)
        self._nodes = None
        self._src32 = self._dst32 = None
        self._seg_cache = {}
        self._process_graph_info(**kwargs)

    # ---- graph-level (batched graph) bookkeeping: pgl/graph.py:1330-1370 -----------------------
    def _process_graph_info(self, **kwargs):
        self._graph_node_index = kwargs.get("_graph_node_index", None)
        self._graph_edge_index = kwargs.get("_graph_edge_index", None)
        self._num_graph = kwargs.get("_num_graph", None)
        if self._num_graph is None:
            self._num_graph = 1
            self._graph_node_index = np.array([0, self._num_nodes], dtype="int64")
            self._graph_edge_index = np.array([0, self.num_edges], dtype="int64")

    def __repr__(self):
        d = {"class": self.__class__.__name__, "num_nodes": int(self.num_nodes),
             "edges_shape": list(self.edges.shape),
             "node_feat": [{"name": k, "shape": list(v.shape), "dtype": str(v.dtype)} for k, v in self.node_feat.items()],
             "edge_feat": [{"name": k, "shape": list(v.shape), "dtype": str(v.dtype)} for k, v in self.edge_feat.items()]}
        return json.dumps(d, ensure_ascii=False)

    # ---- numpy <-> device ---------------------------------------------------------------------
    def is_tensor(self):
        return self._is_tensor

    def _to_tensor_inplace(self, device=None):
        self._edges = to_device_tensor(self._edges, device)
        device = self._edges.device
        if self._edges.dtype != torch.int64:
            self._edges = self._edges.to(torch.int64)
        self._node_feat = {k: to_device_tensor(v, device) for k, v in self._node_feat.items()}
        self._edge_feat = {k: to_device_tensor(v, device) for k, v in self._edge_feat.items()}
        for ix in (self._adj_src_index, self._adj_dst_index):
            if ix is not None and not ix.is_tensor():
                ix.tensor(inplace=True, device=device)
        self._device = device
        self._is_tensor = True
        self._nodes = None
        self._degree_norm_cache = None

    def tensor(self, inplace=True, uva=False, device=None):
        """pgl/graph.py:227-267.  Moves edges, features and any already-built index to the GPU.
        uva: the reference's switch for keeping the graph structure in (pinned) CPU memory while computing on the GPU -- a capacity
        workaround.  Accepted for signature compatibility (it is the reference's SECOND positional argument); the graph goes to HBM
        either way: 288 GB hold every graph the reference's UVA mode was written for (ogbn-papers100M's edge list is 26 GB), and
        the kernels read device memory only.  Like the reference it refuses uva without a GPU."""
        if uva and not torch.cuda.is_available():
            raise ValueError("uva tensor graph should be run under gpu environment!")
        if self._is_tensor:
            return self
        if inplace:
            self._to_tensor_inplace(device)
            return self
        g = self._rebuild(edges=self._edges.copy(), num_nodes=self._num_nodes, node_feat=dict(self._node_feat),
                           edge_feat=dict(self._edge_feat),
                           adj_src_index=None if self._adj_src_index is None else self._adj_src_index.tensor(False, device=device),
                           adj_dst_index=None if self._adj_dst_index is None else self._adj_dst_index.tensor(False, device=device),
                           _num_graph=self._num_graph, _graph_node_index=self._graph_node_index,
                           _graph_edge_index=self._graph_edge_index)
        if not g._is_tensor:
            g._to_tensor_inplace(device)
        return g

    def _rebuild(self, **kw):
        """The copy tensor(inplace=False) / numpy(inplace=False) return: Graph's own constructor arguments (BiGraph translates them)."""
        return self.__class__(**kw)

    def numpy(self, inplace=True):
        """pgl/graph.py:269-300."""
        if not self._is_tensor:
            return self
        conv = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
        edges = conv(self._edges)
        nf = {k: conv(v) for k, v in self._node_feat.items()}
        ef = {k: conv(v) for k, v in self._edge_feat.items()}
        if inplace:
            self._edges, self._node_feat, self._edge_feat = edges, nf, ef
            for ix in (self._adj_src_index, self._adj_dst_index):
                if ix is not None:
                    ix.numpy(inplace=True)
            self._is_tensor, self._device, self._nodes = False, None, None
            self._src32 = self._dst32 = None
            self._seg_cache = {}
            self._csr_views = None
            self._csr_dview = None                   # (index views of the device the graph was on: ADVICE r5)
            self._edge_order_view = None
            self._degree_norm_cache = None           # (device tensors of the graph that was: ADVICE r4)
            self._weight_tables = None
            return self
        return self._rebuild(edges=edges, num_nodes=self._num_nodes, node_feat=nf, edge_feat=ef,
                              adj_src_index=None if self._adj_src_index is None else self._adj_src_index.numpy(False),
                              adj_dst_index=None if self._adj_dst_index is None else self._adj_dst_index.numpy(False),
                              _num_graph=self._num_graph, _graph_node_index=self._graph_node_index,
                              _graph_edge_index=self._graph_edge_index)

    # ---- dump / load: the reference's .npy directory layout (pgl/graph.py:1177-1302) ------------
    def dump(self, path):
        if self._is_tensor:
            return self.numpy(inplace=False).dump(path)
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, "num_nodes.npy"), self._num_nodes)
        np.save(os.path.join(path, "edges.npy"), self._edges)
        np.save(os.path.join(path, "num_graph.npy"), self._num_graph)
        if self._adj_src_index is not None:
            self._adj_src_index.dump(os.path.join(path, "adj_src"))
        if self._adj_dst_index is not None:
            self._adj_dst_index.dump(os.path.join(path, "adj_dst"))
        if self._graph_node_index is not None:
            np.save(os.path.join(path, "graph_node_index.npy"), np.asarray(self._graph_node_index))
        if self._graph_edge_index is not None:
            np.save(os.path.join(path, "graph_edge_index.npy"), np.asarray(self._graph_edge_index))
        for sub, feats in (("node_feat", self._node_feat), ("edge_feat", self._edge_feat)):
            if len(feats) == 0:
                continue
            os.makedirs(os.path.join(path, sub), exist_ok=True)
            for k, v in feats.items():
                np.save(os.path.join(path, sub, k + ".npy"), v)

    def to_mmap(self, path="./tmp"):
        """pgl/graph.py:1297-1302: dump, then reload memory-mapped (shareable between processes)."""
        self.dump(path)
        return Graph.load(path, mmap_mode="r")

    def node_batch_iter(self, batch_size, shuffle=True):
        """pgl/graph.py:1369-1395."""
        if self._is_tensor:
            perm = torch.randperm(self.num_nodes, device=self._edges.device) if shuffle \
                else torch.arange(self.num_nodes, device=self._edges.device)
        else:
            perm = np.arange(self.num_nodes)
            if shuffle:
                np.random.shuffle(perm)
        start = 0
        while start < self.num_nodes:
            yield perm[start:start + batch_size]
            start += batch_size

    @classmethod
    def load(cls, path, mmap_mode="r"):
        num_nodes = int(np.load(os.path.join(path, "num_nodes.npy")))
        edges = np.load(os.path.join(path, "edges.npy"), mmap_mode=mmap_mode)
        num_graph = int(np.load(os.path.join(path, "num_graph.npy")))
        kw = {}
        for name in ("adj_src", "adj_dst"):
            p = os.path.join(path, name)
            kw[name + "_index"] = EdgeIndex.load(p, mmap_mode=mmap_mode) if os.path.isdir(p) else None

        def feats(sub):
            d = os.path.join(path, sub)
            if not os.path.isdir(d):
                return {}
            return {f[:-4]: np.load(os.path.join(d, f), mmap_mode=mmap_mode) for f in sorted(os.listdir(d)) if f.endswith(".npy")}

        for name in ("graph_node_index", "graph_edge_index"):
            f = os.path.join(path, name + ".npy")
            kw["_" + name] = np.load(f, mmap_mode=mmap_mode) if os.path.exists(f) else None
        return cls(edges=edges, num_nodes=num_nodes, node_feat=feats("node_feat"), edge_feat=feats("edge_feat"),
                   _num_graph=num_graph, **kw)

    # ---- basic properties ---------------------------------------------------------------------
    @property
    def num_nodes(self):
        return self._num_nodes

    @property
    def num_edges(self):
        return int(self._edges.shape[0])

    @property
    def edges(self):
        return self._edges

    @property
    def nodes(self):
        if self._nodes is None:
            self._nodes = torch.arange(self._num_nodes, device=self._device) if self._is_tensor else np.arange(self._num_nodes)
        return self._nodes

    @property
    def node_feat(self):
        return self._node_feat

    @property
    def edge_feat(self):
        return self._edge_feat

    @property
    def num_graph(self):
        return self._num_graph

    @property
    def graph_edge_id(self):
        """pgl/graph.py graph_edge_id: graph id of each edge in a batched graph."""
        from .utils.helper import generate_segment_id_from_index
        ids = generate_segment_id_from_index(np.asarray(self._graph_edge_index))
        return to_device_tensor(ids, self._device) if self._is_tensor else ids

    @classmethod
    def disjoint(cls, graph_list, merged_graph_index=False):
        """pgl/graph.py Graph.disjoint: one big graph out of several, node ids offset graph by graph.
        merged_graph_index=True treats the result as ONE graph, False keeps per-graph node/edge ranges
        (graph_node_id / graph_edge_id, used by graph_pool / graph_norm readouts)."""
        assert len(graph_list) > 0, "The input graph_list of Graph.disjoint has length %d. It should be greater than 0. " % len(graph_list)
        is_tensor = graph_list[0].is_tensor()
        cat = (lambda xs: torch.cat(xs, 0)) if is_tensor else (lambda xs: np.concatenate(xs, axis=0))
        offs = np.concatenate([[0], np.cumsum([g.num_nodes for g in graph_list])]).astype("int64")
        eoffs = np.concatenate([[0], np.cumsum([g.num_edges for g in graph_list])]).astype("int64")
        edges = cat([g.edges + int(o) for g, o in zip(graph_list, offs[:-1])])
        def join(feats):
            keys = feats[0].keys()
            return {k: cat([f[k] for f in feats]) for k in keys}
        kw = {}
        if not merged_graph_index:
            kw = dict(_num_graph=len(graph_list), _graph_node_index=offs, _graph_edge_index=eoffs)
        return cls(edges=edges, num_nodes=int(offs[-1]), node_feat=join([g.node_feat for g in graph_list]),
                   edge_feat=join([g.edge_feat for g in graph_list]), **kw)

    @staticmethod
    def batch(graph_list):
        """Alias of Graph.disjoint(graph_list, merged_graph_index=False) (pgl/graph.py:1040-1043)."""
        return Graph.disjoint(graph_list, merged_graph_index=False)

    @property
    def graph_node_id(self):
        """pgl/graph.py graph_node_id: graph id of each node in a batched graph."""
        from .utils.helper import generate_segment_id_from_index
        ids = generate_segment_id_from_index(np.asarray(self._graph_node_index))
        return to_device_tensor(ids, self._device) if self._is_tensor else ids

    @property
    def adj_src_index(self):
        """pgl/graph.py:1307-1316."""
        if self._adj_src_index is None:
            self._adj_src_index = EdgeIndex.from_edges(u=self._edges[:, 0], v=self._edges[:, 1], num_nodes=self._num_nodes,
                                                       check_range=not getattr(self, "_ids_in_range", False))
        return self._adj_src_index

    @property
    def adj_dst_index(self):
        """pgl/graph.py:1319-1328 (u = dst, v = src)."""
        if self._adj_dst_index is None:
            self._adj_dst_index = EdgeIndex.from_edges(u=self._edges[:, 1], v=self._edges[:, 0], num_nodes=self._num_nodes,
                                                       check_range=not getattr(self, "_ids_in_range", False))
        return self._adj_dst_index

    def sorted_edges(self, sort_by="src"):
        """pgl/graph.py:392-413 -> (sorted_src, sorted_dst, sorted_eid)."""
        if sort_by not in ["src", "dst"]:
            raise ValueError("sort_by should be in 'src' or 'dst'.")
        if sort_by == "src":
            src, dst, eid = self.adj_src_index.triples()
        else:
            dst, src, eid = self.adj_dst_index.triples()
        return src, dst, eid

    def indegree(self, nodes=None):
        """pgl/graph.py:427-447."""
        deg = self.adj_dst_index.degree
        if nodes is None:
            return deg
        return ops.gather_rows(deg, to_device_tensor(nodes, self._device)) if self._is_tensor else deg[nodes]

    def outdegree(self, nodes=None):
        """pgl/graph.py:449-469."""
        deg = self.adj_src_index.degree
        if nodes is None:
            return deg
        return ops.gather_rows(deg, to_device_tensor(nodes, self._device)) if self._is_tensor else deg[nodes]

    def successor(self, nodes=None, return_eids=False):
        """pgl/graph.py:475-528 (numpy mode only, as in the reference)."""
        if self.is_tensor():
            raise ValueError("You must call Graph.numpy() first. Tensor object don't supprt successor now.")
        if return_eids:
            return self.adj_src_index.view_v(nodes), self.adj_src_index.view_eid(nodes)
        return self.adj_src_index.view_v(nodes)

    def predecessor(self, nodes=None, return_eids=False):
        """pgl/graph.py:572-626."""
        if self.is_tensor():
            raise ValueError("You must call Graph.numpy() first. Tensor object don't supprt predecessor now.")
        if return_eids:
            return self.adj_dst_index.view_v(nodes), self.adj_dst_index.view_eid(nodes)
        return self.adj_dst_index.view_v(nodes)

    def _sample_from_index(self, index, nodes, max_degree, return_eids, shuffle):
        """Host sampling over a numpy EdgeIndex: all neighbours if degree <= max_degree (optionally
        shuffled), else max_degree of them without replacement -- the contract of
        graph_kernel.sample_subset(_with_eid) (pgl/graph_kernel.pyx:266-339), numpy's RNG as there."""
        if self.is_tensor():
            raise ValueError("You must call Graph.numpy() first. Tensor object don't supprt sampling on the host; "
                             "use pgl_amd.sampling.NeighborSampler for the GPU path.")
        nodes = np.arange(index.degree.shape[0]) if nodes is None else np.asarray(nodes, dtype="int64")
        nbrs, eids = [], []
        for v in nodes:
            b, e = int(index._indptr[v]), int(index._indptr[v + 1])
            if e - b > max_degree:
                pick = b + np.random.choice(e - b, max_degree, replace=False)
            elif shuffle:
                pick = b + np.random.permutation(e - b)
            else:
                pick = np.arange(b, e)
            nbrs.append(np.asarray(index._sorted_v[pick], dtype="int64"))
            eids.append(np.asarray(index._sorted_eid[pick], dtype="int64"))
        return (nbrs, eids) if return_eids else nbrs

    def sample_predecessor(self, nodes, max_degree, return_eids=False, shuffle=False):
        """pgl/graph.py:644-688."""
        return self._sample_from_index(self.adj_dst_index, nodes, max_degree, return_eids, shuffle)

    def sample_successor(self, nodes, max_degree, return_eids=False, shuffle=False):
        """pgl/graph.py:530-570."""
        return self._sample_from_index(self.adj_src_index, nodes, max_degree, return_eids, shuffle)

    def get_segment_ids(self, src, dst, segment_by="dst"):
        """pgl/graph.py:1397-1407 -- cached (uniq_ind, segment_ids) of the sorted key column."""
        if segment_by not in self._seg_cache:
            ix = self.adj_dst_index if segment_by == "dst" else self.adj_src_index
            self._seg_cache[segment_by] = ops.unique_segment(ix.degree, ix.triples()[0])
        return self._seg_cache[segment_by]

    # ---- engine plumbing ----------------------------------------------------------------------
    def _require_tensor(self, msg="You must call Graph.tensor()"):
        if not self._is_tensor:
            raise ValueError(msg)

    def _edge_cols32(self):
        if self._src32 is None:
            self._src32 = ops.narrow_i64(self._edges[:, 0])
            self._dst32 = ops.narrow_i64(self._edges[:, 1])
        return self._src32, self._dst32

    def _csr_dst(self):
        return self.adj_dst_index.csr

    def _csr_src(self):
        return self.adj_src_index.csr

    def _csr_dst_view(self):
        """The dst-keyed half of _csr_order_views alone (no src index is built for it)."""
        if getattr(self, "_csr_views", None) is not None:
            return self._csr_views[0]
        if getattr(self, "_csr_dview", None) is None:
            self._csr_dview = self._csr_dst().view(eid32=None)
        return self._csr_dview

    def _csr_order_views(self):
        """Index views for edge tensors kept in DST-SORTED (CSR) order instead of original edge order: the dst-keyed view
        has no eid indirection at all (position p of the walk is row p of the tensor), the src-keyed view maps each of
        its positions to the dst-sorted position of the same edge.  Layers that own a whole score -> softmax -> weighted
        sum chain keep their [E,H] tensors in this order so that every pass over them is sequential."""
        if getattr(self, "_csr_views", None) is None:
            cd, cs = self._csr_dst(), self._csr_src()
            inv = torch.empty(cd.num_edges, dtype=torch.int32, device=cd.eid32.device)
            inv[cd.eid32.long()] = torch.arange(cd.num_edges, dtype=torch.int32, device=inv.device)
            self._csr_views = (cd.view(eid32=None), cs.view(eid32=inv[cs.eid32.long()].contiguous()))
        return self._csr_views

    def _csr_succ_sorted(self):
        """The successor index the walks follow (pgl/sampling/walk.py reads graph.successor): key = src, every row ascending by
        dst, ties in edge-id order.  Tensor mode: an ops.CSR from two stable passes of ops.csr_build (adj_dst_index's dst-sorted
        order, then keyed by src); numpy mode: (indptr int64, col int32) from np.lexsort((dst, src)).  Cached per graph and mode;
        adj_src_index (rows in edge-id order) is left as it is."""
        cache = getattr(self, "_succ_sorted", None)
        if cache is not None and cache[0] == self._is_tensor and cache[1] == self._device:
            return cache[2]
        if self._is_tensor:
            cd = self._csr_dst()
            val = ops.csr_build(cd.col32.to(torch.int64), cd.row32.to(torch.int64), self._num_nodes, want_i64=False,
                                check_range=False)
        else:
            e = np.asarray(self._edges, dtype=np.int64).reshape(-1, 2)
            order = np.lexsort((e[:, 1], e[:, 0]))
            indptr = np.zeros(self._num_nodes + 1, np.int64)
            np.cumsum(np.bincount(e[:, 0], minlength=self._num_nodes)[:self._num_nodes], out=indptr[1:])
            val = (indptr, np.ascontiguousarray(e[order, 1], dtype=np.int32))
        self._succ_sorted = (self._is_tensor, self._device, val)
        return val

    def _csr_pred_sorted(self):
        """The mirror of _csr_succ_sorted: key = dst, every row ascending by src, ties in edge-id order -- what a membership
        test "is (x, v) an edge" for a fixed tail v searches (sampling.corrupt_edges(side="src")).  Tensor mode: an ops.CSR from
        adj_src_index's src-sorted stream keyed by dst (a stable pass); numpy mode: (indptr int64, col int32) from
        np.lexsort((src, dst)).  Cached per graph and mode; adj_dst_index (rows in edge-id order) is left as it is."""
        cache = getattr(self, "_pred_sorted", None)
        if cache is not None and cache[0] == self._is_tensor and cache[1] == self._device:
            return cache[2]
        if self._is_tensor:
            cs = self._csr_src()
            val = ops.csr_build(cs.col32.to(torch.int64), cs.row32.to(torch.int64), self._num_nodes, want_i64=False,
                                check_range=False)
        else:
            e = np.asarray(self._edges, dtype=np.int64).reshape(-1, 2)
            order = np.lexsort((e[:, 0], e[:, 1]))
            indptr = np.zeros(self._num_nodes + 1, np.int64)
            np.cumsum(np.bincount(e[:, 1], minlength=self._num_nodes)[:self._num_nodes], out=indptr[1:])
            val = (indptr, np.ascontiguousarray(e[order, 0], dtype=np.int32))
        self._pred_sorted = (self._is_tensor, self._device, val)
        return val

    def _succ_edge_ids(self):
        """The ORIGINAL edge id of every position of _csr_succ_sorted() (int32 tensor / int64 array).  Tensor mode: that index
        was built over the dst-sorted stream, so its eid32 addresses dst-sorted positions and is composed with adj_dst_index's
        own eid32; numpy mode: the lexsort that orders the index.  Cached beside the index."""
        cache = getattr(self, "_succ_eids", None)
        if cache is not None and cache[0] == self._is_tensor and cache[1] == self._device:
            return cache[2]
        if self._is_tensor:
            val = ops.gather_rows(self._csr_dst().eid32.reshape(-1, 1), self._csr_succ_sorted().eid32).reshape(-1).contiguous()
        else:
            e = np.asarray(self._edges, dtype=np.int64).reshape(-1, 2)
            val = np.lexsort((e[:, 1], e[:, 0])).astype(np.int64)
        self._succ_eids = (self._is_tensor, self._device, val)
        return val

    def edge_weight_table(self, weight, index="dst"):
        """Engine extension: the ops.WeightTable of per-edge weights over one of this graph's indices -- index="dst": the
        dst-sorted index neighbour sampling reads (ops.sample_neighbors / NeighborSampler weights=); "succ": the sorted successor
        index the walks follow (sampling.walks / random_walk weights=).  weight: the name of an edge_feat entry, or an [E]
        tensor / array in ORIGINAL edge order (this method composes the index's edge permutation).  Tensor graph: built on the
        device and cached per (index, the tensor's storage, offset, length and version counter), like ops.edge_scale -- an
        in-place update of the weights rebuilds it; numpy graph: the host twin, not cached.  ValueError for a NaN, negative or
        infinite weight; zero weights are legal and never drawn."""
        if index not in ("dst", "succ"):
            raise ValueError("edge_weight_table: index must be 'dst' or 'succ'")
        if isinstance(weight, str):
            if weight not in self._edge_feat:
                raise KeyError("edge_weight_table: no edge feature %r" % weight)
            weight = self._edge_feat[weight]
        E = self.num_edges
        if not self._is_tensor:
            w = np.asarray(weight)
            if w.size != E:
                raise ValueError("edge_weight_table: %d weights for %d edges" % (w.size, E))
            if index == "dst":
                ix = self.adj_dst_index
                return ops.host_edge_weight_table(ix._indptr, w.reshape(-1), ix._sorted_eid)
            return ops.host_edge_weight_table(self._csr_succ_sorted()[0], w.reshape(-1), self._succ_edge_ids())
        w = to_device_tensor(weight, self._device)
        if w.numel() != E:
            raise ValueError("edge_weight_table: %d weights for %d edges" % (w.numel(), E))
        w = w.reshape(-1)
        ver = ops.tensor_version(w)
        key = None if ver is None else (index, w.untyped_storage().data_ptr(), w.storage_offset(), w.numel(), ver, str(w.dtype), str(w.device))
        cache = getattr(self, "_weight_tables", None)
        if cache is None or cache[0] != self._device:
            cache = self._weight_tables = (self._device, {})
        hit = cache[1].get(index)
        if key is not None and hit is not None and hit[0] == key:
            return hit[2]
        if index == "dst":
            csr = self._csr_dst()
            table = ops.edge_weight_table(csr, w, csr.eid32)
        else:
            table = ops.edge_weight_table(self._csr_succ_sorted(), w, self._succ_edge_ids())
        if key is not None:                                   # (the entry HOLDS the weights: their address cannot be reused while it lives)
            cache[1][index] = (key, w, table)
        return table

    def edge_order(self, order="dst"):
        """Engine extension: a view of this graph whose EDGE TENSORS ([E, ...]) are kept in destination-sorted (CSR)
        order instead of original edge order.  In original order every pass over an [E, H] tensor that is keyed by
        destination (edge_softmax, send_ue_recv's edge operand) reaches its rows through the eid permutation -- one
        128-byte line per 32-byte row at H = 8; in this order the same passes are sequential.  A user-defined attention
        layer opts in by producing its scores with `view.send_uv` / `view.sddmm`, normalising them with `view.edge_softmax`
        and consuming them with `view.send_ue_recv` -- exactly what the built-in layers do internally; `to_order` /
        `from_order` convert an original-order tensor when one has to cross (one permuted pass each)."""
        if order != "dst":
            raise ValueError("edge_order: only 'dst' is provided")
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        if getattr(self, "_edge_order_view", None) is None:
            self._edge_order_view = _DstOrderedEdges(self)
        return self._edge_order_view

    # ---- message passing (pgl/graph.py:694-966) -------------------------------------------------
    def send(self, message_func, src_feat=None, dst_feat=None, edge_feat=None, node_feat=None):
        """pgl/graph.py:694-776."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor() first")
        if (src_feat is not None or dst_feat is not None) and node_feat is not None:
            raise ValueError("Can not use src/dst feat and node feat at the same time")
        src_feat_temp, dst_feat_temp = {}, {}
        if node_feat is not None:
            assert isinstance(node_feat, dict), "The input node_feat must be a dict"
            src_feat_temp.update(node_feat)
            dst_feat_temp.update(node_feat)
        else:
            if src_feat is not None:
                assert isinstance(src_feat, dict), "The input src_feat must be a dict"
                src_feat_temp.update(src_feat)
            if dst_feat is not None:
                assert isinstance(dst_feat, dict), "The input dst_feat must be a dict"
                dst_feat_temp.update(dst_feat)
        edge_feat_temp = {}
        if edge_feat is not None:
            assert isinstance(edge_feat, dict), "The input edge_feat must be a dict"
            edge_feat_temp.update(edge_feat)
        src32, dst32 = self._edge_cols32()
        view = self.edge_order("dst") if self._lazy_edges(torch.empty(0, device=self._device)) else None
        # (with the EdgeTensor mechanism on, floating features are gathered straight into the engine's destination-sorted edge order
        #  and tagged: element-wise message functions keep the tag, and recv(mode="dst") then needs no permutation of the [E, ...]
        #  messages at all -- the reference permutes every message by eid, pgl/graph.py:821-823)
        src_reader = _GraphRowReader(src_feat_temp, src32, self._csr_src, view, "src")
        dst_reader = _GraphRowReader(dst_feat_temp, dst32, self._csr_dst, view, "dst")
        if view is not None and edge_feat_temp:
            edge_feat_temp = _EdgeFeatReader(edge_feat_temp, view, self)
        msg = message_func(src_reader, dst_reader, edge_feat_temp)
        if not isinstance(msg, dict):
            raise TypeError("The outputs of the %s function is expected to be a dict, but got %s"
                            % (message_func.__name__, type(msg)))
        return msg

    def recv(self, reduce_func, msg, recv_mode="dst"):
        """pgl/graph.py:778-832."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        if not isinstance(msg, dict):
            raise TypeError("The input of msg should be a dict, but receives a %s" % (type(msg)))
        if not callable(reduce_func):
            raise TypeError("reduce_func should be callable")
        src, dst, eid = self.sorted_edges(sort_by=recv_mode)
        csr = self._csr_dst() if recv_mode == "dst" else self._csr_src()
        msg = _SortedAwareReader(msg, csr.eid32, self if recv_mode == "dst" else None)
        uniq_ind, segment_ids = self.get_segment_ids(src, dst, segment_by=recv_mode)
        bucketed_msg = Message(msg, segment_ids, num_segments=int(uniq_ind.shape[0]))
        output = reduce_func(bucketed_msg)
        return ag.scatter_into_zeros(self._num_nodes, uniq_ind, output)

    def send_recv(self, feature, reduce_func="sum", out_size=None):
        """pgl/graph.py:834-861."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        assert reduce_func in _REDUCE, "Only support 'sum', 'mean', 'max', 'min' built-in reduce functions."
        return self._aggregate(feature, None, "add", reduce_func, out_size)

    def send_u_recv(self, feature, reduce_op="sum", out_size=None):
        """pgl/graph.py:863-887."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        assert reduce_op in _REDUCE, "Only support 'sum', 'mean', 'max', 'min' built-in reduce functions."
        return self._aggregate(feature, None, "add", reduce_op, out_size)

    def send_ue_recv(self, feature, edge_feature, message_op="add", reduce_op="sum", out_size=None):
        """pgl/graph.py:889-937."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        assert message_op in _MSGOP, "Only support 'add', 'sub', 'max', 'min' build-in message functions."
        assert reduce_op in _REDUCE, "Only support 'sum', 'mean', 'max', 'min' built-in reduce functions."
        rows = _et.sorted_rows(edge_feature, self)
        if rows is not None:                                     # the operand is already in the order the kernel walks: no eid indirection
            return self.edge_order("dst").send_ue_recv(feature, rows, message_op, reduce_op, out_size)
        return self._aggregate(feature, _et.materialize(edge_feature), message_op, reduce_op, out_size)

    def send_uv(self, src_feature, dst_feature, message_op="add"):
        """pgl/graph.py:939-966."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        assert message_op in _MSGOP, "Only support 'add', 'sub', 'max', 'min' build-in message functions."
        if self._lazy_edges(src_feature):
            # rows produced in the engine's own (destination-sorted) edge order and tagged: leaky_relu / dropout / edge_softmax /
            # send_ue_recv downstream then never touch the eid permutation; whoever READS the values gets original edge order
            view = self.edge_order("dst")
            return _et.EdgeTensor(view.send_uv(src_feature, dst_feature, message_op), view)
        src32, dst32 = self._edge_cols32()
        return ag.send_uv(src_feature, dst_feature, src32, dst32, message_op, self._csr_dst, self._csr_src)

    def _lazy_edges(self, like):
        """True when [E, ...] results of this graph are handed out as EdgeTensors (pgl_amd/edge_tensor.py): a tensor graph on the
        GPU, floating rows, the mechanism not switched off (graph.lazy_edge_order = False / PGLAMD_EDGE_TENSOR=0)."""
        return (_et.ENABLED and getattr(self, "lazy_edge_order", True) and self._is_tensor and isinstance(like, torch.Tensor)
                and like.is_cuda and like.is_floating_point())

    def send_ue(self, feature, edge_feature, message_op="add"):
        raise NotImplementedError

    def sddmm(self, src_feature, dst_feature):
        """alpha[e, h] = <src_feature[src_e, h, :], dst_feature[dst_e, h, :]> for [N, H, D] fp32 inputs: the dot-product
        attention score of every edge in one pass, without the two [E, H, D] gathers a send_uv("mul") + sum would
        materialise (engine extension; differentiable).  Shapes the kernel does not cover fall back to that composition."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        if (src_feature.dim() == 3 and src_feature.dtype == torch.float32 and dst_feature.dtype == torch.float32
                and tuple(src_feature.shape[1:]) == tuple(dst_feature.shape[1:])
                and ops.sddmm_supported(int(src_feature.shape[1]), int(src_feature.shape[2]))):
            if self._lazy_edges(src_feature):
                view = self.edge_order("dst")
                return _et.EdgeTensor(view.sddmm(src_feature, dst_feature), view)
            return ag.sddmm(src_feature.contiguous(), dst_feature.contiguous(), self._csr_dst(), self._csr_src)
        return self.send_uv(src_feature, dst_feature, "mul").sum(-1)

    def send_recv_scaled(self, feature, src_scale=None, dst_scale=None):
        """out[v] = dst_scale[v] * sum_{u->v} src_scale[u] * feature[u] in ONE kernel: GCN's symmetric
        normalisation (pgl/nn/conv.py:242-250) fused into the aggregation (engine extension, fp32)."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        ss = None if src_scale is None else src_scale.reshape(-1).contiguous()
        ds = None if dst_scale is None else dst_scale.reshape(-1).contiguous()
        if ss is not None and ss.numel() != feature.shape[0]:
            raise ValueError("src_scale must hold one value per source node (%d), got %d" % (feature.shape[0], ss.numel()))
        if ds is not None and ds.numel() != feature.shape[0]:
            raise ValueError("dst_scale must hold one value per destination node (%d), got %d" % (feature.shape[0], ds.numel()))
        return ag.aggregate(feature, self._csr_dst(), self._csr_src, "sum", None, None, "add", None, None, ss, ds)

    def send_recv_dense(self, feature, weight, bias=None, act=None, src_scale=None, dst_scale=None, reduce_op="sum"):
        """act( (dst_scale * REDUCE_{u->v} src_scale[u] * feature[u]) @ weight^T + bias ) with the aggregate never leaving the
        chip (engine extension for GCNConv's aggregate -> linear -> bias -> activation, pgl/nn/conv.py:242-254).  fp32,
        feature [N, 64 | 128], weight [d_out, d_in] (nn.Linear layout); differentiable in feature, weight and bias."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        ss = None if src_scale is None else src_scale.reshape(-1).to(feature.dtype).contiguous()   # (applied as one pass over [N, d]:
        ds = None if dst_scale is None else dst_scale.reshape(-1).contiguous()                     #  cheaper than a 4-byte read per edge)
        return ag.aggregate_dense(feature.contiguous(), weight, bias, self._csr_dst(), self._csr_src, act, ds, reduce_op, ss)

    def send_recv_dual_linear(self, feature, w_self, w_neigh, reduce_op="sum"):
        """feature @ w_self^T + send_recv(feature, reduce_op) @ w_neigh^T as one differentiable op (engine extension for GraphSageConv
        in full-graph mode, pgl/nn/conv.py:99-109): the gradient of `feature` is written by one GEMM and accumulated into by the
        transposed aggregation instead of being added up by an extra pass over [N, d].  fp32, sum / mean."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        return ag.aggregate_dual_linear(feature.contiguous(), w_self, w_neigh, self._csr_dst(), self._csr_src, reduce_op)

    def reorder(self, num_clusters=None, rows_per_cluster=4096, seed=0):
        """-> (graph2, order): the same graph with its nodes RENUMBERED cluster by cluster (engine extension, opt-in; the
        reference feeds node ids as they come, pgl/graph.py:859).  order[new_id] = old_id; graph2's node features are
        self's rows taken in that order, edges keep their order (and their features), only their endpoints are relabelled.
        The clusters come from the engine's own multilevel partitioner (pglamd_partition_edges) asked for N / rows_per_cluster
        parts: a cluster's feature rows (4096 x 512 B = 2 MiB at d = 128 fp32) fit the 4 MiB L2 of one XCD, and consecutive
        chunks of the destination-sorted stream then gather from the cluster they are walking, so that a source row is
        fetched from HBM about once per cluster that reads it instead of once per edge.  Results on graph2 are results on
        self up to this relabelling: out2[new] == out[order[new]].  Worth it only where the graph HAS clusters
        (profiles/r04/locality.txt: planted communities yes, RMAT no)."""
        n = self.num_nodes
        k = int(num_clusters) if num_clusters else max(2, -(-n // int(rows_per_cluster)))
        e = self._edges.detach().cpu().numpy() if check_is_tensor(self._edges) else np.asarray(self._edges)
        part, _ = ops.host_partition_edges(e, n, k, None, None, 1.10, 1.10, seed)
        order = np.argsort(part, kind="stable").astype(np.int64)
        new_of_old = np.empty(n, np.int64)
        new_of_old[order] = np.arange(n, dtype=np.int64)
        if self._is_tensor:
            dev = self._edges.device
            order_t, map_t = torch.from_numpy(order).to(dev), torch.from_numpy(new_of_old).to(dev)
            edges2 = map_t[self._edges]
            nf = {key: ops.gather_rows(v, order_t) if v.is_cuda else v[order_t] for key, v in self._node_feat.items()}
            g2 = self.__class__(edges=edges2, num_nodes=n, node_feat=nf, edge_feat=dict(self._edge_feat))
            return g2, order_t
        nf = {key: np.asarray(v)[order] for key, v in self._node_feat.items()}
        return self.__class__(edges=new_of_old[e], num_nodes=n, node_feat=nf, edge_feat=dict(self._edge_feat)), order

    def propagate_step(self, feature, dst_scale, residual=None, residual_scale=0.0):
        """residual_scale * residual + dst_scale (.) (sum over in-edges of feature[src]) in one launch (engine extension
        for the k-hop propagation layers; fp32, dst_scale one value per node)."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        return ag.propagate_step(feature.contiguous(), dst_scale.reshape(-1).contiguous(), self._csr_dst(), self._csr_src,
                                 None if residual is None else residual.contiguous(), float(residual_scale))

    def gat_aggregate(self, feature, attn_src, attn_dst, negative_slope=0.2, attn_drop=0.0, seed=0):
        """send_uv(add) -> leaky_relu -> edge_softmax -> dropout -> send_ue_recv(mul, sum) of GATConv
        (pgl/nn/conv.py:331-339) fused into one pass, differentiable (engine extension; fp32, or an fp16 / bf16 feature: 16-bit
        rows with fp32 sums -- attention_ops.gat16_supported(H, D) -- whose output comes back in the feature's dtype)."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        if feature.dtype in (torch.float16, torch.bfloat16):
            return ag.gat_attention16(feature, attn_src, attn_dst, self._csr_dst(), self._csr_src, negative_slope, attn_drop, seed)
        return ag.gat_attention(feature, attn_src, attn_dst, self._csr_dst(), self._csr_src, negative_slope, attn_drop, seed)

    def dot_attention(self, q, k, v, scale=1.0, attn_drop=0.0, seed=0, edge_feat=None):
        """out[i, h] = sum_{e = (u -> i)} keep_e softmax_i(scale * <q[i, h], k[u, h]>) v[u, h]: the sddmm -> edge_softmax -> dropout
        -> send_ue_recv(mul, sum) chain of TransformerConv (pgl/nn/conv.py:796-847) fused into one pass, differentiable in q, k
        and v (engine extension; fp32 [N, H, D], ops.dot_attention_supported(H, D)).  attn_drop: the in-kernel mask of
        gat_aggregate, drawn from (seed, edge id, head).
        edge_feat (fp32 [num_edges, H, D], ORIGINAL edge order; None: the call above, unchanged): the layer's message function with
        edge features (pgl/nn/conv.py:808-815) in the same pass -- k[u, h] + edge_feat[e, h] in the score, v[u, h] + edge_feat[e, h]
        in the sum -- differentiable in edge_feat as well (attention_ops.dot_attention_edge_supported(H, D))."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        if edge_feat is not None:
            return ag.dot_attention_edge(q, k, v, edge_feat, self._csr_dst(), self._csr_src, float(scale), float(attn_drop), seed)
        return ag.dot_attention(q, k, v, self._csr_dst(), self._csr_src, float(scale), float(attn_drop), seed)

    def gatv2_attention(self, x, attn, negative_slope=0.2, attn_drop=0.0, seed=0, x_dst=None):
        """out[i, h] = sum_{e = (u -> i)} keep_e softmax_i(sum_d attn[h, d] leaky_relu(x[u, h, d] + x_dst[i, h, d])) x[u, h]: the
        send_uv(add) -> leaky_relu -> (. * attn).sum(-1) -> edge_softmax -> dropout -> send_ue_recv(mul, sum) chain of GATv2Conv
        (pgl/nn/conv.py:419-430) fused into one pass, differentiable in x, x_dst and attn (engine extension; fp32 [N, H, D], attn
        [H, D] or [1, H, D], attention_ops.gatv2_attention_supported(H, D)).  x_dst None: x on both sides, as the layer has it.
        attn_drop: the in-kernel mask of gat_aggregate, drawn from (seed, edge id, head).  Applies where dot_attention_rows() does."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        return ag.gatv2_attention(x, x_dst, attn, self._csr_dst(), self._csr_src, float(negative_slope), float(attn_drop), seed)

    def fa_aggregate(self, feature, p_src, p_dst, src_scale=None, dst_scale=None, attn_drop=0.0, seed=0):
        """out[i, h] = sum_{e = (u -> i)} keep_e tanh(p_src[u, h] + p_dst[i, h]) src_scale[u] dst_scale[i] feature[u, h]: the
        send_uv -> tanh -> degree norms -> dropout -> send_ue_recv(mul, sum) chain of FAConv (pgl/nn/conv.py:1306-1339) fused into one
        pass, differentiable in feature, p_src and p_dst (engine extension; fp32, attention_ops.fa_supported(H, D)).  feature: [N, d]
        (one head of d columns) or [N, H, D], and the result has its shape; p_src, p_dst: [N], [N, 1] or [N, H], the two halves of the
        gate's pre-activation; src_scale, dst_scale: one constant per node (no gradient), None: 1.  attn_drop: the in-kernel mask of
        gat_aggregate, drawn from (seed, edge id, head).  Applies where dot_attention_rows() does."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        if feature.dim() not in (2, 3):
            raise ValueError("fa_aggregate: feature must be [N, d] or [N, H, D]")
        n = int(feature.shape[0])
        x = feature.reshape(n, 1, -1) if feature.dim() == 2 else feature
        H = int(x.shape[1])
        f32 = lambda s: None if s is None else s.to(torch.float32)
        out = ag.fa_aggregate(x, p_src.reshape(n, H), p_dst.reshape(n, H), f32(src_scale), f32(dst_scale), self._csr_dst(),
                              self._csr_src, float(attn_drop), seed)
        return out.reshape(feature.shape)

    def dot_attention_rows(self):
        """The number of rows q, k and v of dot_attention must have -- this graph's nodes -- or None where the graph cannot run it (numpy
        mode; a subclass whose sources and destinations are different node sets returns None).  Layers ask this, not the class."""
        return self.num_nodes if self._is_tensor else None

    def gat_aggregate_proj(self, feature, proj, negative_slope=0.2, attn_drop=0.0, seed=0):
        """gat_aggregate with the attention scores computed inside the op: a_src | a_dst = feature.reshape(N, H*D) @ proj (proj
        [H*D, 2H], differentiable).  One autograd node, so the two gradients of `feature` are not added by a separate pass
        (training; engine extension; fp32)."""
        if not self._is_tensor:
            raise ValueError("You must call Graph.tensor()")
        return ag.gat_attention_proj(feature, proj, self._csr_dst(), self._csr_src, negative_slope, attn_drop, seed)

    def _aggregate(self, feature, edge_feature, message_op, reduce_op, out_size):
        if isinstance(out_size, torch.Tensor):
            out_size = int(out_size.item())
        needs_grad = torch.is_grad_enabled() and (feature.requires_grad or
                                                  (edge_feature is not None and edge_feature.requires_grad))
        src32 = dst32 = None
        if needs_grad and (edge_feature is not None or reduce_op in ("max", "min")):
            src32, dst32 = self._edge_cols32()
        return ag.aggregate(feature, self._csr_dst(), self._csr_src, reduce_op, out_size, edge_feature, message_op,
                            src32, dst32)


class _DstOrderedEdges(object):
    """Graph.edge_order("dst"): the graph's message-passing ops for [E, ...] tensors in destination-sorted order.
    Position p of such a tensor is the edge (src[p], dst[p]) = (view.src, view.dst)[p], original id view.eid[p]."""

    def __init__(self, graph):
        self.graph = graph
        self._cd = graph._csr_dst_view()                       # (the src-keyed view -- backward only -- is built on first use: `_cs`)
        self._cs_view = None
        full = graph._csr_dst()
        self.eid = full.eid32                                  # original edge id of position p
        self.src, self.dst = full.col32, full.row32            # endpoints of position p (int32)
        self.num_edges = full.num_edges
        # dst-keyed view with an explicit identity edge map (for the gather-by-edge backward of send_uv)
        self._cd_iota = self._cd.view(eid32=torch.arange(full.num_edges, dtype=torch.int32, device=full.row32.device))
        self._inv = None

    @property
    def _cs(self):
        if self._cs_view is None:
            self._cs_view = self.graph._csr_order_views()[1]
        return self._cs_view

    def to_order(self, edge_tensor):
        """original edge order -> this order (differentiable)."""
        return ag.gather_rows(edge_tensor, self.eid)

    def from_order(self, edge_tensor):
        """this order -> original edge order (differentiable)."""
        if self._inv is None:
            inv = torch.empty(self.num_edges, dtype=torch.int32, device=self.eid.device)
            inv[self.eid.long()] = torch.arange(self.num_edges, dtype=torch.int32, device=inv.device)
            self._inv = inv
        return ag.gather_rows(edge_tensor, self._inv)

    def send_uv(self, src_feature, dst_feature, message_op="add"):
        """Graph.send_uv (pgl/graph.py:939-966), result rows in this order."""
        assert message_op in _MSGOP, "Only support 'add', 'sub', 'max', 'min' build-in message functions."
        return ag.send_uv(src_feature, dst_feature, self.src, self.dst, message_op, lambda: self._cd_iota, lambda: self._cs)

    def sddmm(self, src_feature, dst_feature):
        """Graph.sddmm, result rows in this order."""
        if (src_feature.dim() == 3 and src_feature.dtype == torch.float32 and dst_feature.dtype == torch.float32
                and tuple(src_feature.shape[1:]) == tuple(dst_feature.shape[1:])
                and ops.sddmm_supported(int(src_feature.shape[1]), int(src_feature.shape[2]))):
            return ag.sddmm(src_feature.contiguous(), dst_feature.contiguous(), self._cd, lambda: self._cs)
        return self.send_uv(src_feature, dst_feature, "mul").sum(-1)

    def edge_softmax(self, logits):
        """GF.edge_softmax(graph, logits, norm_by="dst") (pgl/nn/functional/graph_op.py:101-123) for logits in this order:
        the segments are contiguous runs, no permutation is involved."""
        cd = self._cd
        return ag.segment_softmax(logits, ops.SegView(cd.indptr, cd.row32, cd.row32, None))

    def send_ue_recv(self, feature, edge_feature, message_op="add", reduce_op="sum", out_size=None):
        """Graph.send_ue_recv (pgl/graph.py:889-937) with the edge operand in this order."""
        assert message_op in _MSGOP, "Only support 'add', 'sub', 'max', 'min' build-in message functions."
        assert reduce_op in _REDUCE, "Only support 'sum', 'mean', 'max', 'min' built-in reduce functions."
        needs_grad = torch.is_grad_enabled() and (feature.requires_grad or edge_feature.requires_grad)
        s32 = d32 = None
        if needs_grad:
            s32, d32 = self.src, self.dst
        return ag.aggregate(feature, self._cd, lambda: self._cs, reduce_op, out_size, edge_feature, message_op, s32, d32)


class _GraphRowReader(op.RowReader):
    """RowReader whose gathers know the CSR keyed by their index, so backward needs no sort.  With a destination-order view
    (EdgeTensor mechanism on) floating features are gathered in the engine's edge order and handed out tagged."""

    def __init__(self, nfeat, index, csr_fn, view=None, side="src"):
        super(_GraphRowReader, self).__init__(nfeat, index)
        self._csr_fn, self._view, self._side = csr_fn, view, side

    def __getitem__(self, key):
        if key not in self.loaded_nfeat:
            feat = self.nfeat[key]
            v = self._view
            if v is not None and isinstance(feat, torch.Tensor) and feat.is_cuda and feat.is_floating_point():
                if self._side == "src":         # position p of the sorted stream reads its source: backward = the src-keyed view
                    rows = ag.gather_rows(feat, v.src, lambda: v._cs)
                else:                           # ... its destination: a contiguous run per destination row
                    rows = ag.gather_rows(feat, v.dst, lambda: v._cd_iota)
                self.loaded_nfeat[key] = _et.EdgeTensor(rows, v)
            else:
                self.loaded_nfeat[key] = ag.gather_rows(feat, self.index, self._csr_fn)
        return self.loaded_nfeat[key]


class _EdgeFeatReader(dict):
    """The edge features a message function sees: floating ones are permuted into the engine's edge order once (lazily, cached)
    and tagged, so that combining them with gathered node features keeps everything in that order."""

    def __init__(self, feats, view, graph):
        super(_EdgeFeatReader, self).__init__(feats)
        self._view, self._graph, self._done = view, graph, {}

    def __getitem__(self, key):
        if key not in self._done:
            t = dict.__getitem__(self, key)
            if isinstance(t, torch.Tensor) and t.is_cuda and t.is_floating_point() and int(t.shape[0]) == self._view.num_edges:
                t = _et.EdgeTensor(self._view.to_order(t), self._view)
            self._done[key] = t
        return self._done[key]

    def get(self, key, default=None):
        return self[key] if key in self else default


class _SortedAwareReader(op.RowReader):
    """recv's message reader: a message that is an EdgeTensor of this graph already IS in destination-sorted order -- no gather by
    eid; anything else is permuted as the reference does (pgl/graph.py:821-823)."""

    def __init__(self, msg, eid, graph):
        super(_SortedAwareReader, self).__init__(msg, eid)
        self._graph = graph

    def __getitem__(self, key):
        if key not in self.loaded_nfeat:
            val = self.nfeat[key]
            rows = _et.sorted_rows(val, self._graph) if self._graph is not None else None
            if rows is not None:
                self.loaded_nfeat[key] = rows
                return rows
        return super(_SortedAwareReader, self).__getitem__(key)
