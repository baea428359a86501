"""Drop-in for the reference's `models` package (models/__init__.py:1-6).  Only the north-star models are
provided: `models.stgcn` (ST-GCN), its siblings `models.stgin` (graph isomorphism convolution), `models.stpgcn`
(ST-GCN with a projection graph convolution after the first block) and `models.stgcn_debug` (ST-GCN with a trainable
adjacency per frame and per block, the model --freeze-graph-until acts on; the same module holds the layers `GPool`, the top-k
graph pooling that keeps real joints, and `SGCN`, the graph convolution over the per-sample adjacency it emits), `models.resnet` /
`models.resnet18` (VirtualRadar + ResNet-18), the layer-level modules of `models.gcn`, `models.stgcn.TemporalAttention` (the per-frame
gate: an MLP over a frame's V C features ends in a sigmoid that scales the frame), `models.lstm_sampler`
(`TemporalSampler`: an LSTM stack scores the frames of a clip, the top_k best are gathered and scaled by their scores), `models.agcn`
(`AdaptiveAdjacency`, the data-dependent adjacency of 2s-AGCN -- A[k] plus a column softmax of the similarity of two 1x1 embeddings --, and
`AdaptiveGraphConv`, that adjacency followed by `SGCN`), `models.tcn` (`TemporalConv`, a temporal convolution with any kernel size up to
9, dilation up to 8 and stride 1 or 2: the temporal unit of the MS-TCN branches of the later skeleton models), and
`models.stpgcnp` (`ProjectionGraphPool`, the pooling layer of ST-PGCNP; its `Model` is not built yet).
Sub-modules are imported lazily so that `import models` works on a CPU-only box."""
