"""Speaker (dense captioning) head on MI355X: `GraphModule` (EdgeConv relation graph), `TopDownSceneCaptionModule`
(top-down attention two-GRUCell captioner) and `SpeakerNet`, with the reference's constructors, `data_dict` keys and
state-dict layout (reference: model/graph_module.py:21-324, model/caption_module.py:13-898, model/speaker.py:11-52;
SURVEY.md rows A16, A17).

Re-designed hot spots (results unchanged):
  * `_query_locals` for ALL target proposals in one HIP launch (csrc/proposals.hip) instead of 128 sequential calls
    with a device->host->device IoU round trip each (graph_module.py:229-238, 206-210; caption_module.py:821-824);
  * EdgeConv without torch_geometric / scipy: edges = row-major non-zeros of the valid-node adjacency on the device,
    message MLP as two library GEMMs, `index_add_` aggregation (graph_module.py:21-114, 273-277);
  * decode step: embedding row lookup instead of one-hot x table matmul, and `map_feat(obj_feats)` hoisted out of the
    time loop (caption_module.py:95-98, 108 recompute it every step);
  * evaluation decodes all 128 target proposals of a scene as one batch instead of 128 x 31 sequential steps
    (caption_module.py:710-749).
  * self-critical training: the beam search carries only the chosen-token log-probs (not the (N,b,t,V) history),
    keeps per-step snapshots on the device and ranks finished beams with one stable sort (caption_module.py:136-349).
"""
import ctypes as C
import random

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from . import nativelinear
from ._lib import check
from ._call import _on, _ptr, _stream

JOINED_DECODES = True   # the self-critical step's beam search and greedy baseline as one chain (tools/ab.py py:d3net_amd.speaker.JOINED_DECODES=0,1)


# --------------------------------------------------------------------------------------- local context
def query_locals_all(corners, object_masks, num_locals, include_self, overlay_threshold=0.5, query_mode="corner"):
    """Local-context masks of every target proposal: (B,K,8,3), (B,K) -> (B,K,K); row t is what the reference's
    `_query_locals(target_ids = t)` returns (graph_module.py:184-227 / caption_module.py:800-842)."""
    B, K = object_masks.shape
    corners = corners.contiguous().float()
    masks = object_masks.contiguous().float()
    dist = torch.empty((B, K, K), dtype=torch.float32, device=corners.device)
    with _on(corners.device):
        check(_lib.lib().d3_query_locals_dist(_ptr(corners), _ptr(masks), _ptr(dist), B, K, int(include_self),
                                              float(overlay_threshold), int(query_mode == "center"), _stream()),
              "query_locals_dist")
    if NATIVE_TOPK_MASK and K <= 4096:
        out = torch.empty_like(dist)
        with _on(corners.device):      # the L smallest of every row as a 0/1 mask, ties by ascending index like the library's top-k
            check(_lib.lib().d3_query_locals_mask(_ptr(dist), _ptr(out), B * K, K, int(num_locals), _stream()), "query_locals_mask")
        return out
    _, topk_ids = torch.topk(dist, num_locals, largest=False, dim=2)
    return torch.zeros_like(dist).scatter_(2, topk_ids, 1)


NATIVE_TOPK_MASK = True     # False: torch.topk + scatter (tests compare the two)


# ------------------------------------------------------------------------------------------- EdgeConv
class EdgeConv(nn.Module):
    """message = MLP([x_i, x_j - x_i]) summed at the target node i (graph_module.py:21-114).  With the reference's
    edge_index = [adjacency row, adjacency column] and PyG's source->target flow, x_j = x[edge_index[0]] and
    x_i = x[edge_index[1]], aggregation at edge_index[1].  Returns (aggregated nodes, per-edge messages)."""

    def __init__(self, in_size, out_size, aggregation="add"):
        super().__init__()
        assert aggregation == "add"
        self.in_size, self.out_size = in_size, out_size
        self.map_edge = nn.Sequential(nn.Linear(2 * in_size, out_size), nn.ReLU(), nn.Linear(out_size, out_size))

    def forward(self, x, edge_index):
        x_j, x_i = x[edge_index[0]], x[edge_index[1]]
        message = self.map_edge(torch.cat([x_i, x_j - x_i], dim=1))
        out = torch.zeros(x.shape[0], self.out_size, dtype=x.dtype, device=x.device).index_add_(0, edge_index[1], message)
        return out, message


def graph_edges(adjacent_mat, object_masks, num_locals):
    """Edge structures of all scenes in one launch (csrc/edgeconv.hip: d3_graph_edges), fixed-size device tensors."""
    B, K, _ = adjacent_mat.shape
    dev, KL = adjacent_mat.device, K * num_locals
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    e = dict(B=B, K=K, L=num_locals, src=i32(B, KL), dst=i32(B, KL), edge_index=torch.empty((B, 2, KL), dtype=torch.float32, device=dev),
             cnt=i32(B, 4), in_ptr=i32(B, K + 1), in_list=i32(B, KL), out_start=i32(B, K), out_cnt=i32(B, K),
             feat_src=torch.empty((B, KL), dtype=torch.int64, device=dev), pred_src=torch.empty((B, KL), dtype=torch.int64, device=dev))
    adj, masks = adjacent_mat.contiguous().float(), object_masks.contiguous().float()
    with _on(dev):
        check(_lib.lib().d3_graph_edges(_ptr(adj), _ptr(masks), B, K, num_locals, _ptr(e["src"]), _ptr(e["dst"]), _ptr(e["edge_index"]),
                                        _ptr(e["cnt"]), _ptr(e["in_ptr"]), _ptr(e["in_list"]), _ptr(e["out_start"]), _ptr(e["out_cnt"]),
                                        _ptr(e["feat_src"]), _ptr(e["pred_src"]), _stream()), "graph_edges")
    return e


class EdgeConvFunction(torch.autograd.Function):
    """EdgeConv over the padded edge matrix of all scenes (csrc/edgeconv.hip): x (B*K, Cin) -> node (B*K, Cout), per-edge
    messages (B*K*L, Cout; padded rows zero).  One native call each way."""

    @staticmethod
    def forward(ctx, x, W0, b0, W2, b2, e):
        L_ = _lib.lib()
        x, W0, b0, W2, b2 = (t.contiguous() for t in (x, W0, b0, W2, b2))
        B, K, L = e["B"], e["K"], e["L"]
        Cin, Cout = x.shape[1], W2.shape[0]
        Emax = B * K * L
        node = torch.empty((B * K, Cout), dtype=torch.float32, device=x.device)
        msg = torch.empty((Emax, Cout), dtype=torch.float32, device=x.device)
        ws = torch.empty(L_.d3_edgeconv_ws_bytes(Emax, Cin, Cout), dtype=torch.uint8, device=x.device)
        with _on(x.device):
            check(L_.d3_edgeconv_fwd(_ptr(x), _ptr(W0), _ptr(b0), _ptr(W2), _ptr(b2), _ptr(e["src"]), _ptr(e["dst"]), _ptr(e["in_ptr"]),
                                     _ptr(e["in_list"]), B, K, L, Cin, Cout, _ptr(node), _ptr(msg), _ptr(ws), ws.numel(), _stream()),
                  "edgeconv_fwd")
        ctx.e, ctx.dims = e, (Cin, Cout)
        ctx.save_for_backward(W0, W2, ws)
        return node, msg

    @staticmethod
    def backward(ctx, d_node, d_msg):
        L_ = _lib.lib()
        W0, W2, ws = ctx.saved_tensors
        e = ctx.e
        Cin, Cout = ctx.dims
        B, K, L = e["B"], e["K"], e["L"]
        Emax = B * K * L
        dev = W0.device
        d_node = d_node.contiguous() if d_node is not None else None
        d_msg = d_msg.contiguous() if d_msg is not None else None
        dx = torch.empty((B * K, Cin), dtype=torch.float32, device=dev)
        dW0, db0 = torch.empty_like(W0), torch.empty(Cout, dtype=torch.float32, device=dev)
        dW2, db2 = torch.empty_like(W2), torch.empty(Cout, dtype=torch.float32, device=dev)
        ws2 = torch.empty(L_.d3_edgeconv_bwd_ws_bytes(Emax, Cin, Cout), dtype=torch.uint8, device=dev)
        with _on(dev):
            check(L_.d3_edgeconv_bwd(_ptr(W0), _ptr(W2), _ptr(e["src"]), _ptr(e["dst"]), _ptr(e["in_ptr"]), _ptr(e["in_list"]),
                                     _ptr(e["out_start"]), _ptr(e["out_cnt"]), B, K, L, Cin, Cout,
                                     _ptr(d_node) if d_node is not None else None, _ptr(d_msg) if d_msg is not None else None,
                                     _ptr(ws), _ptr(dx), _ptr(dW0), _ptr(db0), _ptr(dW2), _ptr(db2), _ptr(ws2), ws2.numel(), _stream()),
                  "edgeconv_bwd")
        return dx, dW0, db0, dW2, db2, None


class _GatherRowsPad(torch.autograd.Function):
    """rows[idx] with out-of-range entries reading a zero row (csrc/heads.hip: d3_gather_rows_pad); the in-range indices are
    unique, so the backward is the same launch transposed"""

    @staticmethod
    def forward(ctx, rows, idx):
        rows = rows.contiguous()
        idx = idx.contiguous()
        ctx.save_for_backward(idx)
        ctx.shape = rows.shape
        out = torch.empty((idx.numel(), rows.shape[1]), dtype=torch.float32, device=rows.device)
        with _on(rows.device):
            check(_lib.lib().d3_gather_rows_pad(_ptr(rows), rows.shape[0], _ptr(idx), _ptr(out), idx.numel(), rows.shape[1], 0, _stream()),
                  "gather_rows_pad")
        return out

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        g = g.contiguous()
        d = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        with _on(g.device):
            check(_lib.lib().d3_gather_rows_pad(_ptr(g), ctx.shape[0], _ptr(idx), _ptr(d), idx.numel(), ctx.shape[1], 1, _stream()),
                  "gather_rows_pad")
        return d, None


class GraphModule(nn.Module):
    """(reference: model/graph_module.py:116-324)"""

    def __init__(self, in_size, out_size, num_layers, num_proposals, feat_size, num_locals, query_mode="corner",
                 graph_mode="edge_conv", return_edge=False, graph_aggr="add", return_orientation=False, num_bins=6,
                 return_distance=False):
        super().__init__()
        if graph_mode != "edge_conv":
            raise NotImplementedError("graph_mode edge_conv is the only one the reference instantiates (model/speaker.py:21-23)")
        self.in_size, self.out_size = in_size, out_size
        self.num_proposals, self.feat_size, self.num_locals, self.query_mode = num_proposals, feat_size, num_locals, query_mode
        self.map_input = nn.Linear(in_size, out_size)
        self.graph_mode = graph_mode
        self.gc_layers = nn.ModuleList(EdgeConv(out_size, out_size, graph_aggr) for _ in range(num_layers))
        self.return_edge, self.return_orientation, self.return_distance, self.num_bins = return_edge, return_orientation, return_distance, num_bins
        if self.return_orientation:
            self.edge_layer = EdgeConv(out_size, out_size, graph_aggr)
            self.edge_predict = nn.Linear(out_size, num_bins + 1)

    native = True    # csrc/edgeconv.hip for all scenes at once; False: the per-scene library-op form (tests compare the two)

    def _forward_native(self, data_dict, obj_feats, object_masks, adjacent_mat):
        """all scenes as one padded edge matrix: no python loop over scenes, no host round trip (see csrc/edgeconv.hip)"""
        B, K, Cc = obj_feats.shape
        L = self.num_locals
        e = graph_edges(adjacent_mat, object_masks, L)
        node, msg = obj_feats.reshape(B * K, Cc), None
        for layer in self.gc_layers:
            m = layer.map_edge
            node, msg = EdgeConvFunction.apply(node, m[0].weight, m[0].bias, m[2].weight, m[2].bias, e)
        valid = (object_masks == 1).unsqueeze(-1)
        data_dict["bbox_feature"] = torch.where(valid, obj_feats + node.view(B, K, -1), torch.zeros_like(obj_feats))   # (:311-312)
        if self.return_orientation and msg is not None:
            # padded placement of the messages / predictions: an index past the end reads a zero row (no zero-row concat copy)
            edge_feats = _GatherRowsPad.apply(msg, e["feat_src"].view(-1)).view(B, K, L, self.out_size)

            def orientation_head():
                m = self.edge_layer.map_edge
                _, last = EdgeConvFunction.apply(node, m[0].weight, m[0].bias, m[2].weight, m[2].bias, e)
                pred = nativelinear.linear(last, self.edge_predict.weight, self.edge_predict.bias)
                return _GatherRowsPad.apply(pred, e["pred_src"].view(-1)).view(B, K * L, self.num_bins + 1)
            if DEFER_ORIENTATION_HEAD and data_dict.get("_defer_orientation_head"):
                # only the orientation LOSS reads these predictions: SpeakerNet.forward enqueues them behind the captioner's
                # recurrence (its ~300 launches keep the device busy for longer than the host needs to issue them; here, between
                # ScoreNet and the recurrence, the device waits for the host)
                data_dict["_orientation_head"] = orientation_head
                edge_preds = None
            else:
                edge_preds = orientation_head()
            edge_indices = e["edge_index"]
            num_sources, num_targets = e["cnt"][:, 1].long(), e["cnt"][:, 2].long()
        else:
            edge_feats = obj_feats.new_zeros(B, K, L, self.out_size)
            edge_preds = obj_feats.new_zeros(B, K * L, self.num_bins + 1)
            edge_indices = torch.zeros_like(e["edge_index"])
            num_sources = torch.zeros(B, dtype=torch.long, device=obj_feats.device)
            num_targets = torch.zeros(B, dtype=torch.long, device=obj_feats.device)
        data_dict["adjacent_mat"] = adjacent_mat
        data_dict["edge_index"] = edge_indices
        data_dict["edge_feature"] = edge_feats
        data_dict["num_edge_source"] = num_sources
        data_dict["num_edge_target"] = num_targets
        if edge_preds is not None:
            data_dict["edge_orientations"] = edge_preds[:, :, :-1]
            data_dict["edge_distances"] = edge_preds[:, :, -1]
        return data_dict

    def forward(self, data_dict):
        obj_feats = nativelinear.linear(data_dict["proposal_feats_batched"], self.map_input.weight, self.map_input.bias)   # (B,K,out)
        object_masks = data_dict["proposal_batch_mask"]
        B, K, _ = obj_feats.shape
        adjacent_mat = query_locals_all(data_dict["proposal_bbox_batched"], object_masks, self.num_locals,
                                        include_self=False, query_mode=self.query_mode).type_as(object_masks)
        if self.native and obj_feats.is_cuda and self.out_size == self.feat_size:
            return self._forward_native(data_dict, obj_feats, object_masks, adjacent_mat)
        new_obj_feats = obj_feats.new_zeros(B, K, self.feat_size)
        edge_indices = obj_feats.new_zeros(B, 2, K * self.num_locals)
        edge_feats = obj_feats.new_zeros(B, K, self.num_locals, self.out_size)
        edge_preds = obj_feats.new_zeros(B, K * self.num_locals, self.num_bins + 1)
        num_sources = torch.zeros(B, dtype=torch.long, device=obj_feats.device)
        num_targets = torch.zeros(B, dtype=torch.long, device=obj_feats.device)
        for b in range(B):
            valid = object_masks[b] == 1
            sub = adjacent_mat[b][valid][:, valid]
            edge_index = torch.nonzero(sub, as_tuple=False).t().contiguous()        # row-major non-zeros == scipy COO order
            x = obj_feats[b, valid]
            node, message = x, None
            for layer in self.gc_layers:
                node, message = layer(node, edge_index)
            if self.return_orientation and edge_index.shape[1] > 0:
                n_src = int(torch.unique(edge_index[0]).numel())
                n_tar = int(message.shape[0] / n_src)
                n = n_src * n_tar
                num_sources[b], num_targets[b] = n_src, n_tar
                if n_tar <= self.num_locals and n_src <= K:
                    edge_feats[b, :n_src, :n_tar] = message[:n].view(n_src, n_tar, self.out_size)
                    edge_indices[b, :, :n] = edge_index[:, :n].to(edge_indices.dtype)
                    _, last = self.edge_layer(node, edge_index)
                    pred = self.edge_predict(last)
                    if pred.shape[0] == n:      # the reference's assignment raises otherwise and the exception is swallowed (:291-308)
                        edge_preds[b, :n] = pred
            new_obj_feats[b, valid] = x + node                                      # skip connection (:311-312)
        data_dict["bbox_feature"] = new_obj_feats
        data_dict["adjacent_mat"] = adjacent_mat
        data_dict["edge_index"] = edge_indices
        data_dict["edge_feature"] = edge_feats
        data_dict["num_edge_source"] = num_sources
        data_dict["num_edge_target"] = num_targets
        data_dict["edge_orientations"] = edge_preds[:, :, :-1]
        data_dict["edge_distances"] = edge_preds[:, :, -1]
        return data_dict


# ------------------------------------------------------------------------------------------- captioner
_TD_KEYS = {"W_td": "map_topdown.weight", "b_td": "map_topdown.bias", "Wih1": "recurrent_cell_1.weight_ih",
            "Whh1": "recurrent_cell_1.weight_hh", "bih1": "recurrent_cell_1.bias_ih", "bhh1": "recurrent_cell_1.bias_hh",
            "W_feat": "map_feat.weight", "W_hidd": "map_hidd.weight", "w_att": "attend.weight", "W_lang": "map_lang.weight",
            "b_lang": "map_lang.bias", "Wih2": "recurrent_cell_2.weight_ih", "Whh2": "recurrent_cell_2.weight_hh",
            "bih2": "recurrent_cell_2.bias_ih", "bhh2": "recurrent_cell_2.bias_hh", "Wc0": "classifier.0.weight",
            "bc0": "classifier.0.bias", "Wc2": "classifier.2.weight", "bc2": "classifier.2.bias"}
_TD_GETTERS = None


def _td_params(cap):
    """the captioner's parameters in csrc/topdown.hip's argument order (attribute walks: `dict(named_parameters())` per call cost
    ~50 us of interpreter time in a host-bound stretch of the step)"""
    global _TD_GETTERS
    if _TD_GETTERS is None:
        import operator
        _TD_GETTERS = [operator.attrgetter(_TD_KEYS[k]) for k in _lib.TOPDOWN_PARAMS]
    return [g(cap) for g in _TD_GETTERS]


class TopDownXEFunction(torch.autograd.Function):
    """The teacher-forced captioner pass (caption_module.py:636-668: S x `step`) as ONE native call each way
    (csrc/topdown.hip: d3_topdown_xe_forward / _backward).  Inputs: obj_feats (N,K,F), target_feats (N,F), then the 19
    parameters in `_lib.TOPDOWN_PARAMS` order; non-differentiable: embeddings (V,E), word_ids (N,Tw) int64, masks (N,K), S.
    Returns logits (N,S,V) and the attention maps (N,K,S) (`topdown_attn`, not differentiated -- no loss reads it)."""

    @staticmethod
    def forward(ctx, emb, word_ids, masks, S, obj_feats, target_feats, *params):
        L = _lib.lib()
        obj_feats, target_feats, masks = obj_feats.contiguous(), target_feats.contiguous(), masks.contiguous().float()
        word_ids = word_ids.contiguous()
        params = tuple(p.contiguous() for p in params)
        N, K, F_ = obj_feats.shape
        V, E = emb.shape
        H = params[_lib.TOPDOWN_PARAMS.index("W_hidd")].shape[0]
        dev = obj_feats.device
        if not 1 <= S <= word_ids.shape[1]:
            # (the step-by-step form indexes word_ids[:, step] and raises; lang_len must be the CAPTION length here, not the
            # listener's description length)
            raise IndexError("teacher forcing needs %d input words per sample, word_ids has %d" % (S, word_ids.shape[1]))
        a = _lib.TopdownArgs()
        a.N, a.K, a.S, a.V, a.H, a.E, a.F, a.Tw = N, K, S, V, H, E, F_, word_ids.shape[1]
        a.word_ids, a.emb, a.target, a.obj, a.mask = (t.data_ptr() for t in (word_ids, emb, target_feats, obj_feats, masks))
        for k, p in zip(_lib.TOPDOWN_PARAMS, params):
            setattr(a, k, p.data_ptr())
        logits = torch.empty((N, S, V), dtype=torch.float32, device=dev)
        attn = torch.empty((N, K, S), dtype=torch.float32, device=dev)
        ws = torch.empty(L.d3_topdown_ws_bytes(N, K, S, H, E, F_), dtype=torch.uint8, device=dev)
        a.logits, a.attn, a.ws, a.ws_bytes = logits.data_ptr(), attn.data_ptr(), ws.data_ptr(), ws.numel()
        with _on(dev):
            check(L.d3_topdown_xe_forward(C.byref(a), _stream()), "topdown_xe_forward")
        ctx.args = a
        ctx.keep = (emb, word_ids, masks, obj_feats, target_feats, params, ws)
        ctx.mark_non_differentiable(attn)
        return logits, attn

    @staticmethod
    def backward(ctx, dlogits, _dattn):
        L = _lib.lib()
        a = ctx.args
        emb, word_ids, masks, obj_feats, target_feats, params, ws = ctx.keep
        dev = obj_feats.device
        dlogits = dlogits.contiguous()
        g = _lib.TopdownGrads()
        g.dlogits = dlogits.data_ptr()
        grads = [torch.empty_like(p) for p in params]
        for k, t in zip(_lib.TOPDOWN_PARAMS, grads):
            setattr(g, "d" + k, t.data_ptr())
        dobj, dtarget = torch.empty_like(obj_feats), torch.empty_like(target_feats)
        ws2 = torch.empty(L.d3_topdown_bwd_ws_bytes(a.N, a.K, a.S, a.V, a.H, a.E, a.F), dtype=torch.uint8, device=dev)
        g.dobj, g.dtarget, g.ws, g.ws_bytes = dobj.data_ptr(), dtarget.data_ptr(), ws2.data_ptr(), ws2.numel()
        side = _param_grad_stream(dev, params)
        if side is None:
            with _on(dev):
                check(L.d3_topdown_xe_backward(C.byref(a), C.byref(g), _stream()), "topdown_xe_backward")
            return (None, None, None, None, dobj, dtarget) + tuple(grads)
        # Parameter-gradient work on a second stream (csrc/topdown.hip: d3_topdown_xe_backward_ex): the caller's stream goes on with
        # the relation graph's / ScoreNet's / the backbone's backward as soon as dobj / dtarget are enqueued.  The join -- and the
        # release of every buffer the side stream reads -- happens when the autograd engine finishes this backward pass.
        main = torch.cuda.current_stream(dev)
        with _on(dev):
            check(L.d3_topdown_xe_backward_ex(C.byref(a), C.byref(g), C.c_void_p(main.cuda_stream), C.c_void_p(side.cuda_stream)),
                  "topdown_xe_backward_ex")
        done = torch.cuda.Event()
        done.record(side)
        # (NOT the gradient tensors: autograd's AccumulateGrad adopts a gradient only while nobody else holds it and would otherwise
        # copy it on the caller's stream at once -- before the side stream has written it; adopted, p.grad keeps it alive)
        keep = [ctx.keep, dlogits, ws2, a, g]

        def join():
            main.wait_event(done)
            keep.clear()
        torch.autograd.Variable._execution_engine.queue_callback(join)
        return (None, None, None, None, dobj, dtarget) + tuple(grads)


DEFER_ORIENTATION_HEAD = 1   # (A/B switch) XE training: the relation graph's orientation head (read by the orientation loss only) is enqueued behind the captioner's recurrence
PARAM_GRAD_STREAM = 0     # 1: the captioner's parameter-gradient GEMMs on a second stream (d3_topdown_xe_backward_ex; measured neutral on the 4-scene step -- 17.18 vs 17.21 ms, gpurun_out/r05_j19: the caller's stream is host-bound behind the captioner -- so off)
_PG_STREAMS = {}


def _param_grad_stream(dev, params):
    """the side stream of TopDownXEFunction.backward, or None when the overlap is not safe: a parameter that already holds a gradient
    (accumulation reads the new one at once, on the caller's stream) or a data-parallel job (the heads' gradient bucket is all-reduced
    from inside the backward: distributed.BucketGradAllReduce.boundary)"""
    if not PARAM_GRAD_STREAM or any(p.grad is not None for p in params):
        return None
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return None
    key = dev.index
    if key not in _PG_STREAMS:
        _PG_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _PG_STREAMS[key]


class _BeamResult(list):
    """beam_decode's per-sample lists + (native search only) `logp_sums`: the summed log-probability of every returned beam, one
    tensor on the autograd graph, rows in the order of the flattened lists"""
    logp_sums = None
    rows = None


class _NativeDecoder:
    """Inference-time decode loop state for csrc/topdown.hip's d3_topdown_step: map_feat(obj) computed once, hidden states
    double-buffered on the device, 8 launches per step.  obj_feats: (N / obj_div, K, F) -- `obj_div` consecutive samples share
    an object block (the evaluation decode runs the K targets of a scene as K samples: caption_module.py:710-749)."""

    def __init__(self, cap, target_feats, obj_feats, masks, obj_div=1):
        L = _lib.lib()
        self.dev = dev = target_feats.device
        self.target, self.obj, self.mask = target_feats.contiguous().float(), obj_feats.contiguous().float(), masks.contiguous().float()
        N, F_ = self.target.shape
        nblk, K, _ = self.obj.shape
        assert nblk * obj_div == N and self.mask.shape == (N, K)
        self.params = [p.detach().contiguous() for p in _td_params(cap)]
        self.emb = cap.embeddings
        V, E = self.emb.shape
        H = cap.hidden_size
        a = self.args = _lib.TopdownArgs()
        a.N, a.K, a.S, a.V, a.H, a.E, a.F, a.Tw = N, K, 1, V, H, E, F_, 1
        a.emb, a.target, a.obj, a.mask = self.emb.data_ptr(), self.target.data_ptr(), self.obj.data_ptr(), self.mask.data_ptr()
        for k, p in zip(_lib.TOPDOWN_PARAMS, self.params):
            setattr(a, k, p.data_ptr())
        self.obj_div = obj_div
        self.fp = torch.empty((nblk * K, H), dtype=torch.float32, device=dev)
        with _on(dev):
            check(L.d3_topdown_feat_proj(_ptr(self.obj), _ptr(self.params[_lib.TOPDOWN_PARAMS.index("W_feat")]), _ptr(self.fp),
                                         nblk * K, H, F_, _stream()), "topdown_feat_proj")
        self.h1 = [torch.zeros((N, H), device=dev), torch.empty((N, H), device=dev)]
        self.h2 = [torch.zeros((N, H), device=dev), torch.empty((N, H), device=dev)]
        self.ws = torch.empty(L.d3_topdown_step_ws_bytes(N, K, H, E, F_), dtype=torch.uint8, device=dev)
        self.N, self.K, self.V = N, K, V

    def step(self, word):
        """word (N) int64 -> logits (N,V), attention (N,K); advances the hidden states"""
        word = word.contiguous()
        logits = torch.empty((self.N, self.V), dtype=torch.float32, device=self.dev)
        attn = torch.empty((self.N, self.K), dtype=torch.float32, device=self.dev)
        with _on(self.dev):
            check(_lib.lib().d3_topdown_step(C.byref(self.args), _ptr(word), _ptr(self.fp), self.obj_div, _ptr(self.h1[0]), _ptr(self.h2[0]),
                                             _ptr(self.h1[1]), _ptr(self.h2[1]), _ptr(logits), _ptr(attn), _ptr(self.ws), self.ws.numel(),
                                             _stream()), "topdown_step")
        self.h1.reverse(); self.h2.reverse()
        return logits, attn


def _aabb_iou(c1, c2):
    """lib/utils/bbox.py:247-271 on (...,8,3) tensors"""
    mn1, mx1, mn2, mx2 = c1.min(-2)[0], c1.max(-2)[0], c2.min(-2)[0], c2.max(-2)[0]
    inter = (torch.minimum(mx1, mx2) - torch.maximum(mn1, mn2)).clamp(min=0).prod(-1)
    return inter / ((mx1 - mn1).prod(-1) + (mx2 - mn2).prod(-1) - inter + 1e-8)


class _CaptionInputs(torch.autograd.Function):
    """Per-description inputs of the captioner straight from the per-scene tensors (csrc/proposals.hip: d3_caption_inputs_*):
    obj (N,K,F) = bbox_feature[scene] (+ the target's edge features on its adjacency-row neighbours, caption_module.py:866-885),
    target_feats (N,F) = bbox_feature[scene, target], valid (N,K) = the target's local-context mask row.  No per-description
    copies of the (B,K,L,F) edge features / (B,K,K) masks, no masked_scatter; the backward sums a scene's descriptions in
    order (deterministic)."""

    @staticmethod
    def forward(ctx, base, edge, adj, locals_, target_ids, per_scene):
        ctx.set_materialize_grads(False)      # (an output nobody differentiates through arrives as None, not as a zero tensor: one fill launch less each)
        B, K, Fd = base.shape
        N = target_ids.numel()
        dev = base.device
        L = edge.shape[2] if edge is not None else 1
        base_c = base.contiguous()
        edge_c = edge.contiguous() if edge is not None else None
        adj_c = adj.contiguous().float() if edge is not None else None
        loc_c = locals_.contiguous().float() if locals_ is not None else None
        tid = target_ids.contiguous()
        obj = torch.empty((N, K, Fd), dtype=torch.float32, device=dev)
        tf = torch.empty((N, Fd), dtype=torch.float32, device=dev)
        valid = torch.empty((N, K), dtype=torch.float32, device=dev) if loc_c is not None else None
        nbr = torch.empty((N, L), dtype=torch.int32, device=dev)
        with _on(dev):
            check(_lib.lib().d3_caption_inputs_fwd(_ptr(base_c), _ptr(edge_c) if edge_c is not None else None,
                                                   _ptr(adj_c) if adj_c is not None else None,
                                                   _ptr(loc_c) if loc_c is not None else None, _ptr(tid), N, per_scene, K, L, Fd,
                                                   _ptr(obj), _ptr(tf), _ptr(valid) if valid is not None else None, _ptr(nbr), _stream()),
                  "caption_inputs_fwd")
        ctx.save_for_backward(tid, nbr)
        ctx.dims = (B, K, L, Fd, N, per_scene, edge is not None)
        if valid is None:
            valid = torch.empty(0, device=dev)
        ctx.mark_non_differentiable(valid)
        return obj, tf, valid

    @staticmethod
    def backward(ctx, g_obj, g_tf, _g_valid):
        tid, nbr = ctx.saved_tensors
        B, K, L, Fd, N, per_scene, has_edge = ctx.dims
        dev = tid.device
        if g_obj is None:
            g_obj = torch.zeros((N, K, Fd), dtype=torch.float32, device=dev)
        g_obj = g_obj.contiguous()
        g_tf = g_tf.contiguous() if g_tf is not None else None
        d_base = torch.empty((B, K, Fd), dtype=torch.float32, device=dev)
        d_edge = torch.zeros((B, K, L, Fd), dtype=torch.float32, device=dev) if has_edge else None
        with _on(dev):
            check(_lib.lib().d3_caption_inputs_bwd(_ptr(g_obj), _ptr(g_tf) if g_tf is not None else None, _ptr(tid), _ptr(nbr), N,
                                                   per_scene, K, L, Fd, _ptr(d_base), _ptr(d_edge) if d_edge is not None else None,
                                                   _stream()), "caption_inputs_bwd")
        return d_base, d_edge, None, None, None, None


class TopDownSceneCaptionModule(nn.Module):
    """(reference: model/caption_module.py:13-898)"""

    def __init__(self, cfg, vocabulary, embeddings, emb_size=300, feat_size=128, hidden_size=512, num_proposals=256,
                 num_locals=-1, query_mode="corner", use_relation=False, use_oracle=False):
        super().__init__()
        self.cfg, self.vocabulary = cfg, vocabulary
        self.num_vocabs = len(vocabulary["word2idx"])
        self.register_buffer("embeddings", torch.as_tensor(embeddings, dtype=torch.float32))
        self.emb_size, self.feat_size, self.hidden_size = emb_size, feat_size, hidden_size
        self.num_proposals, self.num_locals, self.query_mode = num_proposals, num_locals, query_mode
        self.use_relation, self.use_oracle = use_relation, use_oracle
        self.map_topdown = nn.Linear(hidden_size + feat_size + emb_size, emb_size)
        self.recurrent_cell_1 = nn.GRUCell(input_size=emb_size, hidden_size=hidden_size)
        self.map_feat = nn.Linear(feat_size, hidden_size, bias=False)
        self.map_hidd = nn.Linear(hidden_size, hidden_size, bias=False)
        self.attend = nn.Linear(hidden_size, 1, bias=False)
        self.map_lang = nn.Linear(feat_size + hidden_size, emb_size)
        self.recurrent_cell_2 = nn.GRUCell(input_size=emb_size, hidden_size=hidden_size)
        self.classifier = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.ReLU(), nn.Linear(hidden_size, self.num_vocabs))
        self.native = True   # csrc/topdown.hip for the teacher-forced pass; False: the step-by-step library-op form (tests)

    def forward(self, data_dict, use_tf=True, use_rl=False, is_eval=False, beam_opt={}):
        if is_eval:
            return self._forward_scene_batch(data_dict, beam_opt)
        return self._forward_sample_batch(data_dict, use_tf, use_rl, beam_opt=beam_opt)

    # ---- one decode step (:72-133); `feat_proj` = map_feat(obj_feats), hoisted by the drivers
    def step(self, step_word_idx, hiddens, target_feat, obj_feats, object_masks, feat_proj=None):
        hidden_1, hidden_2 = hiddens
        step_input = self.embeddings[step_word_idx]                               # == one-hot @ embeddings (:95-98)
        step_input = self.map_topdown(torch.cat([step_input, hidden_2, target_feat], dim=-1))
        hidden_1 = self.recurrent_cell_1(step_input, hidden_1)
        if feat_proj is None:
            feat_proj = self.map_feat(obj_feats)
        combined = torch.tanh(feat_proj + self.map_hidd(hidden_1).unsqueeze(1))
        scores = self.attend(combined).masked_fill(object_masks == 0, 0)          # masked scores are 0, not -inf (:112-114)
        masks = F.softmax(scores, dim=1)
        attended = (obj_feats * masks).sum(1)
        hidden_2 = self.recurrent_cell_2(self.map_lang(torch.cat([attended, hidden_1], dim=-1)), hidden_2)
        step_output = self.classifier(hidden_2)
        return step_output, step_output.clone(), (hidden_1, hidden_2), masks

    @torch.no_grad()
    def greedy_decode(self, target_feats, obj_feats, valid_masks, max_len):
        """(:350-383) -> trimmed token / log-prob lists"""
        N = target_feats.shape[0]
        word = torch.full((N,), int(self.vocabulary["word2idx"]["sos"]), dtype=torch.long, device=target_feats.device)
        outs, lps = [], []
        if self.native and target_feats.is_cuda:
            dec = _NativeDecoder(self, target_feats, obj_feats, valid_masks.reshape(N, -1))
            # the whole loop is one library call (d3_topdown_greedy: per step the 8 launches of the decode step + arg-max and its
            # log-softmax value in one launch, written straight into the (max_len, N) outputs)
            L = _lib.lib()
            dev = target_feats.device
            words = torch.empty(max_len, N, dtype=torch.long, device=dev)
            lpa = torch.empty(max_len, N, dtype=torch.float32, device=dev)
            logits = torch.empty((N, self.num_vocabs), dtype=torch.float32, device=dev)
            attn = torch.empty((N, dec.K), dtype=torch.float32, device=dev)
            with _on(dev):
                check(L.d3_topdown_greedy(C.byref(dec.args), _ptr(dec.fp), 1, _ptr(dec.h1[0]), _ptr(dec.h2[0]), _ptr(dec.h1[1]), _ptr(dec.h2[1]),
                                          _ptr(logits), _ptr(attn), _ptr(dec.ws), dec.ws.numel(), _ptr(word), max_len, _ptr(words), _ptr(lpa),
                                          _stream()), "topdown_greedy")
            return self.trim_outputs(words.t().contiguous().unsqueeze(1), lpa.t().contiguous().unsqueeze(1))
        hiddens = (target_feats.new_zeros(N, self.hidden_size), target_feats.new_zeros(N, self.hidden_size))
        proj = self.map_feat(obj_feats)
        for _ in range(max_len):
            _, logits, hiddens, _ = self.step(word, hiddens, target_feats, obj_feats, valid_masks, proj)
            lp, word = F.log_softmax(logits, dim=-1).max(-1)
            outs.append(word.unsqueeze(1)); lps.append(lp.unsqueeze(1))
        return self.trim_outputs(torch.cat(outs, 1).unsqueeze(1), torch.cat(lps, 1).unsqueeze(1))

    def beam_decode(self, target_feats, obj_feats, valid_masks, beam_size, max_len, topn=None):
        """Differentiable batched beam search (:136-349 with the reference's call `opt={"beam_size": b}`: one group, no
        diversity / constraints / temperature).  Returns, per sample, its finished beams best-first as dicts
        {"seq": (l,) tokens, "logps": (l,) log-prob of every chosen token -- on the autograd graph, "p": float}.

        Same search as the reference's, restructured: the b live beams of all N samples advance as one (N*b) batch;
        instead of carrying the full (N,b,t,V) log-prob history and gathering the chosen tokens afterwards
        (:202-204, 609), only the chosen-token log-probs (N,b,t) are carried; finished beams are not copied out one by
        one on the host (:285-300) -- each step keeps its (seq, logps, p, ended) snapshot on the device and the
        per-sample ranking is one stable sort at the end (ties keep the reference's append order: step, then beam).
        """
        if self.native and target_feats.is_cuda:
            return self._beam_decode_native(target_feats, obj_feats, valid_masks, beam_size, max_len, topn)
        N, b, V = target_feats.shape[0], beam_size, self.num_vocabs
        dev = target_feats.device
        eos = int(self.vocabulary["word2idx"]["eos"])
        word = torch.full((N,), int(self.vocabulary["word2idx"]["sos"]), dtype=torch.long, device=dev)
        hiddens = (obj_feats.new_zeros(N, self.hidden_size), obj_feats.new_zeros(N, self.hidden_size))
        proj = self.map_feat(obj_feats)
        _, logits, hiddens, _ = self.step(word, hiddens, target_feats, obj_feats, valid_masks, proj)
        logp = F.log_softmax(logits, dim=-1).view(N, 1, V)                 # t = 0: a single live beam per sample (:176-179)
        # per-beam copies of the context for t >= 1 (== target_feat[inter_ids] etc., :305-307)
        rep = lambda t: t.repeat_interleave(b, dim=0)
        tf_b, of_b, vm_b, proj_b = rep(target_feats), rep(obj_feats), rep(valid_masks), rep(proj)
        base = torch.arange(N, device=dev).unsqueeze(1)
        sums = obj_feats.new_zeros(N, 1)
        seq = torch.zeros(N, b, 0, dtype=torch.long, device=dev)
        lps = obj_feats.new_zeros(N, b, 0)
        snaps = []
        for t in range(max_len):
            live = logp.shape[1]
            cand = (sums.unsqueeze(-1) + logp).reshape(N, live * V)
            ix = torch.sort(cand, -1, True)[1][:, :b]                       # full sort as the reference (:181-182)
            beam_ix, tok = ix // V, ix % V
            state_ix = (beam_ix + base * live).reshape(-1)
            if t > 0:
                seq = seq.gather(1, beam_ix.unsqueeze(-1).expand_as(seq))
                lps = lps.gather(1, beam_ix.unsqueeze(-1).expand_as(lps))
            chosen = logp.reshape(N, live * V).gather(1, ix)
            seq = torch.cat([seq, tok.unsqueeze(-1)], -1)
            lps = torch.cat([lps, chosen.unsqueeze(-1)], -1)
            sums = sums.gather(1, beam_ix) + chosen
            hiddens = tuple(h[state_ix] for h in hiddens)
            ended = (tok == eos) if t < max_len - 1 else torch.ones_like(tok, dtype=torch.bool)
            snaps.append((seq, lps, sums.detach().clone(), ended))
            sums = sums - 1000.0 * ended.to(sums.dtype)                     # finished beams stay, heavily penalised (:300)
            if t == max_len - 1:
                break                                                       # (the reference runs one more, unused, step)
            _, logits, hiddens, _ = self.step(tok.reshape(-1), hiddens, tf_b, of_b, vm_b, proj_b)
            logp = F.log_softmax(logits, dim=-1).view(N, b, V)
        # rank the finished beams of every sample: p descending, stable in (step, beam) order
        P = torch.stack([torch.where(e, p, torch.full_like(p, float("-inf"))) for (_, _, p, e) in snaps], 1).reshape(N, -1)
        keep = b if topn is None else min(topn, b)
        order = torch.sort(P, dim=1, descending=True, stable=True)[1][:, :b].cpu()
        Pc = P.cpu()
        done = []
        for n in range(N):
            beams = []
            for j in order[n].tolist()[:keep]:
                if Pc[n, j] == float("-inf"):
                    break
                t, v = divmod(j, b)
                beams.append({"seq": snaps[t][0][n, v], "logps": snaps[t][1][n, v], "p": float(Pc[n, j])})
            done.append(beams)
        return done

    def _beam_decode_native(self, target_feats, obj_feats, valid_masks, beam_size, max_len, topn=None, greedy_len=0):
        """The same search on the native decode step (csrc/topdown.hip), in two parts:
          1. the search itself runs without autograd on `d3_topdown_step` -- the b beams of a sample are b rows that share the
             sample's object block, a beam re-ordering is a row gather of the two hidden states;
          2. the log-probabilities of the beams that are returned (the `topn` best per sample) are recomputed with gradients by
             ONE teacher-forced pass over those token sequences (`TopDownXEFunction`): a finished beam's hidden-state trajectory is
             exactly the trajectory of feeding its own tokens from the start (re-ordering copies ancestors' states), so values and
             gradients are those of differentiating through the search (the choices themselves carry no gradient) -- without
             keeping 30 steps x b beams of library-op autograd nodes alive."""
        N, b, V = target_feats.shape[0], beam_size, self.num_vocabs
        dev = target_feats.device
        sos, eos = int(self.vocabulary["word2idx"]["sos"]), int(self.vocabulary["word2idx"]["eos"])
        vm = valid_masks.reshape(N, -1)
        rs = b + 1 if greedy_len else b                     # rows per sample: the b beams (+ the greedy row of the joined decode)
        with torch.no_grad():
            dec = _NativeDecoder(self, target_feats.detach().repeat_interleave(rs, dim=0), obj_feats.detach(),
                                 vm.repeat_interleave(rs, dim=0), obj_div=rs)
            word = torch.full((N * rs,), sos, dtype=torch.long, device=dev)
            # The search is ONE library call (d3_topdown_beam): per step the decode step's 8 launches and one selection launch
            # (d3_beam_select: log_softmax, the b best of live * V candidates best first -- what the reference's full descending sort
            # keeps (:181-182); an exact tie between two candidates' float scores is the only way the two could order differently --,
            # token histories, running sums with the -1000 penalty of finished beams (:300), ended flags, and the re-ordering of the
            # hidden states: rows are (sample, beam slot)).  ~25 library launches per step before round 4, then a host loop of two
            # calls per step, now none.  With `greedy_len` the greedy baseline of the same samples (:350-383) rides in the same chain
            # as one more row per sample (d3_topdown_beam_greedy).
            L = _lib.lib()
            allseq = torch.zeros(max_len, N, b, max_len, dtype=torch.long, device=dev)   # every step's beams, zero padded
            snap_all = torch.empty(max_len, N, b, dtype=torch.float32, device=dev)
            ended_all = torch.empty(max_len, N, b, dtype=torch.uint8, device=dev)
            sums = [torch.zeros(N, b, dtype=torch.float32, device=dev), torch.empty(N, b, dtype=torch.float32, device=dev)]
            tok = torch.empty(N * rs, dtype=torch.long, device=dev)
            h1 = [dec.h1[0], dec.h1[1], torch.empty_like(dec.h1[0])]
            h2 = [dec.h2[0], dec.h2[1], torch.empty_like(dec.h2[0])]
            logits = torch.empty((N * rs, V), dtype=torch.float32, device=dev)
            attn = torch.empty((N * rs, dec.K), dtype=torch.float32, device=dev)
            P3 = C.c_void_p * 3
            with _on(dev):
                if greedy_len:
                    g_words = torch.empty(greedy_len, N, dtype=torch.long, device=dev)
                    g_lps = torch.empty(greedy_len, N, dtype=torch.float32, device=dev)
                    check(L.d3_topdown_beam_greedy(C.byref(dec.args), _ptr(dec.fp), b, P3(*[t.data_ptr() for t in h1]), P3(*[t.data_ptr() for t in h2]),
                                                   _ptr(logits), _ptr(attn), _ptr(dec.ws), dec.ws.numel(), _ptr(word), eos, max_len, _ptr(allseq),
                                                   _ptr(snap_all), _ptr(ended_all), _ptr(sums[0]), _ptr(sums[1]), _ptr(tok), greedy_len,
                                                   _ptr(g_words), _ptr(g_lps), _stream()), "topdown_beam_greedy")
                else:
                    check(L.d3_topdown_beam(C.byref(dec.args), _ptr(dec.fp), b, P3(*[t.data_ptr() for t in h1]), P3(*[t.data_ptr() for t in h2]),
                                            _ptr(logits), _ptr(attn), _ptr(dec.ws), dec.ws.numel(), _ptr(word), eos, max_len, _ptr(allseq),
                                            _ptr(snap_all), _ptr(ended_all), _ptr(sums[0]), _ptr(sums[1]), _ptr(tok), _stream()), "topdown_beam")
            P = torch.where(ended_all.bool(), snap_all, torch.full_like(snap_all, float("-inf"))).permute(1, 0, 2).reshape(N, -1)
            keep = b if topn is None else min(topn, b)
            order = torch.sort(P, dim=1, descending=True, stable=True)[1][:, :b].cpu()
            Pc = P.cpu()
        picked = []                                                         # (sample, step, beam slot, p)
        for n in range(N):
            for j in order[n].tolist()[:keep]:
                if Pc[n, j] == float("-inf"):
                    break
                t, v = divmod(j, b)
                picked.append((n, t, v, float(Pc[n, j])))
        done = _BeamResult([] for _ in range(N))
        if greedy_len:
            greedy = self.trim_outputs(g_words.t().contiguous().unsqueeze(1), g_lps.t().contiguous().unsqueeze(1))
        if not picked:
            return (done, greedy) if greedy_len else done
        # teacher-forced replay of the returned beams: inputs [sos, tok_0 .. tok_{l-2}] predict tok_0 .. tok_{l-1}
        R, S = len(picked), max(t + 1 for _, t, _, _ in picked)
        pk = torch.tensor([(n, t, v) for n, t, v, _ in picked], dtype=torch.long).to(dev)
        rows = pk[:, 0]
        toks = allseq[pk[:, 1], pk[:, 0], pk[:, 2], :S]                      # (R, S), zero behind a beam's own length
        word_ids = torch.cat([torch.full((R, 1), sos, dtype=torch.long, device=dev), toks], 1)   # (R, S + 1)
        logits, _ = TopDownXEFunction.apply(self.embeddings, word_ids, vm.index_select(0, rows), S, obj_feats.index_select(0, rows),
                                            target_feats.index_select(0, rows), *_td_params(self))
        lp = F.log_softmax(logits, dim=-1).gather(2, toks.unsqueeze(-1)).squeeze(-1)              # (R, S)
        # every returned beam's summed log-probability in one masked reduction, rows in (sample, rank) order: what the self-critical
        # loss needs (loss_helper.py:128-131 sums each list entry: one slice + one reduction + their backward launches per caption)
        done.logp_sums = (lp * (torch.arange(S, device=dev).unsqueeze(0) <= pk[:, 1].unsqueeze(1)).to(lp.dtype)).sum(1)
        done.rows = [(n, t) for n, t, _, _ in picked]
        for r, (n, t, v, p_) in enumerate(picked):
            done[n].append({"seq": toks[r, :t + 1], "logps": lp[r, :t + 1], "p": p_})
        return (done, greedy) if greedy_len else done

    def trim_outputs(self, raw_word_ids, raw_logprobs):
        """cut every sequence at its first eos / pad_ (:385-414); if none occurs the LAST token is dropped, as the
        reference's loop leaves t = max_len - 1"""
        eos, pad = int(self.vocabulary["word2idx"]["eos"]), int(self.vocabulary["word2idx"]["pad_"])
        ids, lps = raw_word_ids.cpu(), raw_logprobs.cpu()
        N, topn, T = ids.shape
        out_ids, out_lps = [], []
        for n in range(N):
            a, b = [], []
            for s in range(topn):
                stop = ((ids[n, s] == eos) | (ids[n, s] == pad)).nonzero()
                t = int(stop[0]) if len(stop) else T - 1
                a.append(raw_word_ids[n, s, :t]); b.append(raw_logprobs[n, s, :t])
            out_ids.append(a); out_lps.append(b)
        return out_ids, out_lps

    def select_target(self, bbox_objness, bbox_center, bbox_corner, bbox_center_label, bbox_corner_label, ref_box_label,
                      ref_box_corner_label, is_annotated, bbox_id_label=None, not_annotated=None):
        """(:416-508) target proposal per description: best IoU with the referred box when annotated, else a random
        non-empty proposal (python `random`, one draw per such sample, in sample order) assigned to its nearest GT.
        The proposal / GT tensors are PER SCENE ((B,K,.), (B,G,.)); description n belongs to scene n // (N // B) -- the
        reference replicates them per description first."""
        N = ref_box_corner_label.shape[0]
        B, K, _ = bbox_center.shape
        per = N // B
        if self.use_oracle:
            raise NotImplementedError("use_oracle (model.no_detection) is off in every shipped config")
        if self.native and bbox_corner.is_cuda and bbox_corner.dtype == torch.float32:
            dev = bbox_corner.device
            ref_box_label = ref_box_label.float()
            target_ids = torch.empty(N, dtype=torch.int64, device=dev)
            labels = torch.empty(N, dtype=torch.int64, device=dev)
            target_ious = torch.empty(N, dtype=torch.float32, device=dev)
            with _on(dev):   # one launch: IoU of the referred box with the scene's K proposals, first maximum; label arg-max
                check(_lib.lib().d3_caption_select_target(_ptr(bbox_corner.contiguous()), _ptr(ref_box_corner_label.contiguous().float()),
                                                          _ptr(ref_box_label.contiguous()), N, per, K, ref_box_label.shape[1],
                                                          _ptr(target_ids), _ptr(target_ious), _ptr(labels), _stream()),
                      "caption_select_target")
        else:
            bidx = torch.arange(N, device=bbox_corner.device) // per
            ious = _aabb_iou(bbox_corner.index_select(0, bidx), ref_box_corner_label.unsqueeze(1))          # (N,K)
            ann_ids = ious.argmax(1)
            target_ids, target_ious = ann_ids.clone(), ious.gather(1, ann_ids.unsqueeze(1)).squeeze(1)
            labels = ref_box_label.argmax(-1)
        # (`not_annotated`: their number when the caller already knows it -- 0 saves the host round trip)
        not_ann = [] if not_annotated == 0 else (is_annotated != 1).nonzero().view(-1).tolist()
        if not_ann:
            objness = bbox_objness.cpu()
            for n in not_ann:
                b = n // per
                valid = (objness[b] == 1).nonzero().view(-1)
                pool = valid if len(valid) > 0 else torch.arange(K)
                t = int(pool[random.randrange(len(pool))])                         # == random.choice(valid_ids)
                d = ((bbox_center[b, t].unsqueeze(0) - bbox_center_label[b]) ** 2).sum(-1)   # nn_distance default (squared L2)
                a = int(d.argmin())
                target_ids[n], labels[n] = t, a
                target_ious[n] = _aabb_iou(bbox_corner[b, t], bbox_corner_label[b, a])
        return target_ids, target_ious, labels

    def _query_locals(self, corners, target_ids, object_masks, include_self=True, overlay_threshold=0.5):
        """(:800-842) -> (N,K) local-context mask of the given targets"""
        allm = query_locals_all(corners, object_masks, self.num_locals, include_self, overlay_threshold, self.query_mode)
        return allm.gather(1, target_ids.view(-1, 1, 1).expand(-1, 1, allm.shape[2])).squeeze(1)

    def _add_relation_feat(self, rel_feats, adjacent_mat, obj_feats, target_ids):
        """(:866-885) add the target's edge features onto its adjacency-row neighbours, in ascending slot order"""
        N = rel_feats.shape[0]
        rel = rel_feats.gather(1, target_ids.view(N, 1, 1, 1).expand(-1, 1, self.num_locals, self.feat_size)).squeeze(1)
        rows = adjacent_mat.gather(1, target_ids.view(N, 1, 1).expand(-1, 1, self.num_proposals)).squeeze(1)
        rel_masks = rows.unsqueeze(-1).expand(-1, -1, self.feat_size) == 1
        return obj_feats + torch.zeros_like(obj_feats).masked_scatter(rel_masks, rel)

    # ---- training driver (:510-687)
    def _forward_sample_batch(self, data_dict, use_tf, use_rl, beam_opt={}):
        K, L = self.num_proposals, self.num_locals
        word_ids = data_dict["lang_ids"].reshape(-1, self.cfg.data.max_spk_len + 2)
        des_lens = data_dict["lang_len"].reshape(-1)
        is_annotated = data_dict["annotated"].reshape(-1)
        ref_labels = data_dict["ref_box_label"].reshape(-1, 128)
        ref_corners = data_dict["ref_box_corner_label"].reshape(-1, 8, 3)
        N = des_lens.shape[0]
        Cn = N // data_dict["center_label"].shape[0]
        rep = lambda t: t.unsqueeze(1).repeat(1, Cn, *([1] * (t.dim() - 1))).reshape(N, *t.shape[1:])
        obj_masks = rep(data_dict["proposal_batch_mask"])
        # ONE host round trip for the two scalars the driver needs: the longest description and whether any sample lacks an
        # annotation (the reference reads both separately: des_lens.max(), and a python loop over is_annotated)
        meta = data_dict.pop("_spk_host_meta", None)     # (PipelineNet.training_step asked for them at the start of the step)
        num_words, n_not_ann = meta.get() if meta is not None else torch.stack([des_lens.max().long(), (is_annotated != 1).sum()]).tolist()

        target_ids, target_ious, labels = self.select_target(
            data_dict["proposal_batch_mask"], data_dict["proposal_center_batched"], data_dict["proposal_bbox_batched"],
            data_dict["center_label"], data_dict["gt_bbox"], ref_labels, ref_corners, is_annotated, not_annotated=n_not_ann)
        data_dict["assigned_bbox_id_labels"] = labels
        allm = None
        if L != -1:   # one launch for the B scenes, then the rows of the N targets
            allm = query_locals_all(data_dict["proposal_bbox_batched"], data_dict["proposal_batch_mask"], L, True, 0.5, self.query_mode)
        base = data_dict["bbox_feature"]
        if self.native and base.is_cuda and base.dtype == torch.float32 and self.feat_size % 4 == 0:
            # per-description inputs straight from the per-scene tensors (no (N,K,L,F) / (N,K,K) copies, no masked_scatter)
            obj_feats, target_feats, vm = _CaptionInputs.apply(base, data_dict["edge_feature"] if self.use_relation else None,
                                                               data_dict["adjacent_mat"] if self.use_relation else None, allm,
                                                               target_ids, Cn)
            valid_masks = vm if allm is not None else obj_masks
        else:
            obj_feats = rep(base)
            target_feats = obj_feats.gather(1, target_ids.view(N, 1, 1).expand(-1, 1, self.feat_size)).squeeze(1)
            valid_masks = obj_masks if allm is None else rep(allm).gather(1, target_ids.view(N, 1, 1).expand(-1, 1, K)).squeeze(1)
            if self.use_relation:
                obj_feats = self._add_relation_feat(rep(data_dict["edge_feature"]), rep(data_dict["adjacent_mat"]), obj_feats, target_ids)
        valid_masks = valid_masks.unsqueeze(-1)

        if use_rl:   # self-critical: sampled = best beams (with gradients), baseline = greedy (:588-633)
            assert beam_opt
            beam_size, topn = beam_opt.get("train_beam_size", 5), beam_opt.get("train_sample_topn", 1)
            if JOINED_DECODES and self.native and target_feats.is_cuda:
                # both decodes of the step in one chain of launches (csrc/topdown.hip d3_topdown_beam_greedy)
                done, (greedy, _) = self._beam_decode_native(target_feats, obj_feats, valid_masks, beam_size, self.cfg.data.max_spk_len, topn,
                                                             greedy_len=self.cfg.data.max_spk_len + 1)
            else:
                done = self.beam_decode(target_feats, obj_feats, valid_masks, beam_size, self.cfg.data.max_spk_len, topn)
                greedy, _ = self.greedy_decode(target_feats, obj_feats, valid_masks, self.cfg.data.max_spk_len + 1)
            lang_cap = [[done[n][k]["seq"] for k in range(topn)] for n in range(N)]
            data_dict["lang_logprob"] = [[done[n][k]["logps"] for k in range(topn)] for n in range(N)]
            sums = getattr(done, "logp_sums", None)
            if sums is not None and sums.shape[0] == N * topn and all(len(done[n]) == topn for n in range(N)):
                data_dict["lang_logprob_sum"] = sums          # == [lp.sum() for beams in lang_logprob for lp in beams], one reduction
            data_dict["baseline_cap"] = [[greedy[n][0] for _ in range(topn)] for n in range(N)]
        elif use_tf and self.native and obj_feats.is_cuda:
            # teacher forcing: every input word is known up front -> the whole S-step pass is one native call (csrc/topdown.hip)
            lang_cap, data_dict["topdown_attn"] = TopDownXEFunction.apply(
                self.embeddings, word_ids, valid_masks.squeeze(-1), max(num_words, 2) - 1, obj_feats, target_feats, *_td_params(self))
        else:
            hiddens = (obj_feats.new_zeros(N, self.hidden_size), obj_feats.new_zeros(N, self.hidden_size))
            proj = self.map_feat(obj_feats)
            outputs, masks = [], []
            word = word_ids[:, 0]
            for step_id in range(1, max(num_words, 2)):
                logits, _, hiddens, m = self.step(word, hiddens, target_feats, obj_feats, valid_masks, proj)
                outputs.append(logits.unsqueeze(1)); masks.append(m)
                word = word_ids[:, step_id] if use_tf else logits.argmax(-1)
            data_dict["topdown_attn"] = torch.cat(masks, dim=-1)
            lang_cap = torch.cat(outputs, dim=1)
        good = target_ious > self.cfg.data.min_iou_threshold
        data_dict["lang_cap"] = lang_cap
        gf = good.to(target_ious.dtype)          # == target_ious[good].mean() (0 when no box is good), without the host round trip
        data_dict["pred_ious"] = (target_ious * gf).sum() / gf.sum().clamp(min=1)
        data_dict["valid_masks"] = valid_masks
        data_dict["good_bbox_masks"] = good
        return data_dict

    # ---- evaluation driver (:689-770): all K targets of every scene decoded as one batch of B*K
    @torch.no_grad()
    def _forward_scene_batch(self, data_dict, beam_opt={}):
        K, L = self.num_proposals, self.num_locals
        obj_feats, obj_masks = data_dict["bbox_feature"], data_dict["proposal_batch_mask"]
        B = obj_feats.shape[0]
        T = self.cfg.data.max_spk_len + 1
        if L == -1:
            valid = obj_masks.unsqueeze(1).expand(-1, K, -1)
        else:
            valid = query_locals_all(data_dict["proposal_bbox_batched"], obj_masks, L, True, 0.5, self.query_mode)
        target_ids = torch.arange(K, device=obj_feats.device).repeat(B)
        feats = obj_feats.unsqueeze(1).expand(-1, K, -1, -1).reshape(B * K, K, self.feat_size)
        step_feats = feats
        if self.use_relation:
            rel = data_dict["edge_feature"].unsqueeze(1).expand(-1, K, -1, -1, -1).reshape(B * K, K, L, self.feat_size)
            adj = data_dict["adjacent_mat"].unsqueeze(1).expand(-1, K, -1, -1).reshape(B * K, K, K)
            step_feats = self._add_relation_feat(rel, adj, feats, target_ids)
        # NOTE the reference builds prop_obj_feats with the relation features but then feeds the plain obj_feats to
        # step() (caption_module.py:713,719,738): the relation features do not reach the evaluation decode.
        del step_feats
        target_feats = obj_feats.reshape(B * K, self.feat_size)
        vm = valid.reshape(B * K, K, 1)
        word = torch.full((B * K,), int(self.vocabulary["word2idx"]["sos"]), dtype=torch.long, device=feats.device)
        outs, attn = [], []
        if self.native and obj_feats.is_cuda:   # B*K samples, the K targets of a scene share its object block (no expand)
            dec = _NativeDecoder(self, target_feats, obj_feats, valid.reshape(B * K, K), obj_div=K)
            for _ in range(T):
                logits, m = dec.step(word)
                word = logits.argmax(-1)
                outs.append(word.unsqueeze(1)); attn.append(m.unsqueeze(-1))
        else:
            hiddens = (feats.new_zeros(B * K, self.hidden_size), feats.new_zeros(B * K, self.hidden_size))
            proj = self.map_feat(obj_feats).unsqueeze(1).expand(-1, K, -1, -1).reshape(B * K, K, self.hidden_size)
            for _ in range(T):
                logits, _, hiddens, m = self.step(word, hiddens, target_feats, feats, vm, proj)
                word = logits.argmax(-1)
                outs.append(word.unsqueeze(1)); attn.append(m)
        data_dict["lang_cap"] = torch.cat(outs, 1).view(B, K, T)
        data_dict["topdown_attn"] = torch.cat(attn, -1).view(B, K, K, T)
        data_dict["valid_masks"] = valid
        return data_dict


class SpeakerNet(nn.Module):
    """(reference: model/speaker.py:11-52)"""

    def __init__(self, cfg, vocabulary, embeddings):
        super().__init__()
        self.cfg, self.vocabulary, self.embeddings = cfg, vocabulary, embeddings
        if cfg.model.num_graph_steps > 0:
            self.graph = GraphModule(cfg.model.m, 128, cfg.model.num_graph_steps, cfg.model.max_num_proposal, 128,
                                     cfg.model.num_locals, return_edge=cfg.model.use_relation,
                                     return_orientation=cfg.model.use_orientation)
        if not cfg.model.no_captioning:
            self.caption = TopDownSceneCaptionModule(cfg, vocabulary, embeddings, num_proposals=cfg.model.max_num_proposal,
                                                     num_locals=cfg.model.num_locals, use_relation=cfg.model.use_relation,
                                                     use_oracle=cfg.model.no_detection)

    def forward(self, data_dict, use_tf=True, use_rl=False, is_eval=False, beam_opt={}):
        if self.cfg.model.num_graph_steps > 0:
            # (training with teacher forcing: the graph's orientation head may run behind the captioner, see GraphModule._forward_native)
            defer = bool(DEFER_ORIENTATION_HEAD) and self.training and use_tf and not use_rl and not is_eval and not self.cfg.model.no_captioning
            if defer:
                data_dict["_defer_orientation_head"] = True
            data_dict = self.graph(data_dict)
            data_dict.pop("_defer_orientation_head", None)
            from .pointgroup import _mark
            _mark("graph")
        if not self.cfg.model.no_captioning:
            data_dict = self.caption(data_dict, use_tf, use_rl, is_eval, beam_opt)
        head = data_dict.pop("_orientation_head", None)
        if head is not None:
            edge_preds = head()
            data_dict["edge_orientations"] = edge_preds[:, :, :-1]
            data_dict["edge_distances"] = edge_preds[:, :, -1]
        return data_dict
