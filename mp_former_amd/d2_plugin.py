"""Registry binding of the two HIP decoders (the plugin boundary B3 / B4 of SURVEY.md 8(b)).

The reference selects its decoders BY NAME from two registries:

* the pixel decoder from detectron2's ``SEM_SEG_HEADS_REGISTRY`` (mask2former/modeling/pixel_decoder/fpn.py:21-34,
  ``build_pixel_decoder``: ``SEM_SEG_HEADS_REGISTRY.get(cfg.MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME)(cfg, input_shape)``);
* the transformer decoder from ``TRANSFORMER_DECODER_REGISTRY``
  (mask2former/modeling/transformer_decoder/maskformer_transformer_decoder.py:16-28, ``build_transformer_decoder``:
  ``TRANSFORMER_DECODER_REGISTRY.get(cfg.MODEL.MASK_FORMER.TRANSFORMER_DECODER_NAME)(cfg, in_channels, mask_classification)``).

``register()`` adds ``MSDeformAttnPixelDecoderHIP`` and ``MultiScaleMaskedTransformerDecoderMaskDNHIP`` to them, so that a
stock MP-Former checkout runs the HIP path with two config overrides (run_50ep_no_noise_all_ly.sh:18-21):

    MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME MSDeformAttnPixelDecoderHIP
    MODEL.MASK_FORMER.TRANSFORMER_DECODER_NAME MultiScaleMaskedTransformerDecoderMaskDNHIP

Importing this module registers when detectron2 and mask2former are importable and is a no-op otherwise (this image has
neither: ``registered()`` is then False and tests/test_host_logic_cpu.py drives ``register`` with stub registries of
detectron2's ``Registry`` interface).  The construction convention of the registries — ``cls(cfg, ...)`` resolved through
``cls.from_config`` — is detectron2's ``@configurable``; where detectron2 is absent the same call convention is provided by
``_configurable`` below, so the registered classes behave identically in both worlds.

The backbone is selected the same way from detectron2's ``BACKBONE_REGISTRY`` (``MODEL.BACKBONE.NAME``): ``register_backbone()``
adds ``D2SwinTransformerHIP`` (swin.py, native shifted-window attention) there; the override is
``MODEL.BACKBONE.NAME D2SwinTransformerHIP``.

The training input of the COCO-instance configuration can be formed on the device as well: ``COCOInstanceLSJDeviceMapper`` is the
worker side of the reference's LSJ mapper (it only reads the image and draws the geometry) and ``install_native_lsj`` the model
side (augment.py: one resample launch and one polygon pass per batch).
"""
import functools

from . import pixel_decoder as _P
from . import transformer_decoder as _T

PIXEL_DECODER_NAME = "MSDeformAttnPixelDecoderHIP"
TRANSFORMER_DECODER_NAME = "MultiScaleMaskedTransformerDecoderMaskDNHIP"

_registered = False


def _looks_like_cfg(x):
    """detectron2.config.config._called_with_cfg: a CfgNode (or anything with its attribute tree) in first position / as `cfg`."""
    return hasattr(x, "MODEL") and not isinstance(x, (int, float, str, dict, list, tuple))


def _configurable(init):
    """detectron2.config.configurable for ``__init__``: ``cls(cfg, *args)`` -> ``cls(**cls.from_config(cfg, *args))``;
    explicit keyword construction passes through."""
    @functools.wraps(init)
    def wrapped(self, *args, **kwargs):
        cfg = args[0] if args else kwargs.get("cfg")
        if _looks_like_cfg(cfg):
            init(self, **type(self).from_config(*args, **kwargs))
        else:
            init(self, *args, **kwargs)
    return wrapped


def make_classes(configurable=None):
    """The two registrable subclasses; ``configurable`` = detectron2's decorator when it is there."""
    deco = configurable or _configurable

    class MSDeformAttnPixelDecoderHIP(_P.MSDeformAttnPixelDecoder):
        @deco
        def __init__(self, *a, **k):
            super().__init__(*a, **k)

    class MultiScaleMaskedTransformerDecoderMaskDNHIP(_T.MultiScaleMaskedTransformerDecoderMaskDN):
        @deco
        def __init__(self, *a, **k):
            super().__init__(*a, **k)

    MSDeformAttnPixelDecoderHIP.__name__ = MSDeformAttnPixelDecoderHIP.__qualname__ = PIXEL_DECODER_NAME
    MultiScaleMaskedTransformerDecoderMaskDNHIP.__name__ = MultiScaleMaskedTransformerDecoderMaskDNHIP.__qualname__ = TRANSFORMER_DECODER_NAME
    return MSDeformAttnPixelDecoderHIP, MultiScaleMaskedTransformerDecoderMaskDNHIP


def register(sem_seg_heads_registry=None, transformer_decoder_registry=None, configurable=None):
    """Register both classes.  Without arguments: detectron2's ``SEM_SEG_HEADS_REGISTRY`` and mask2former's
    ``TRANSFORMER_DECODER_REGISTRY`` (returns False, registering nothing, when either package is missing).  With
    arguments: any two objects with detectron2's ``Registry`` interface (``register(obj)`` / ``get(name)``).
    Returns the two classes (truthy) on success."""
    global _registered
    if sem_seg_heads_registry is None or transformer_decoder_registry is None:
        try:
            from detectron2.config import configurable as d2_configurable
            from detectron2.modeling import SEM_SEG_HEADS_REGISTRY
            from mask2former.modeling.transformer_decoder.maskformer_transformer_decoder import TRANSFORMER_DECODER_REGISTRY
        except ImportError:
            return False
        sem_seg_heads_registry = sem_seg_heads_registry or SEM_SEG_HEADS_REGISTRY
        transformer_decoder_registry = transformer_decoder_registry or TRANSFORMER_DECODER_REGISTRY
        configurable = configurable or d2_configurable
        default = True
    else:
        default = False
    pix, dec = make_classes(configurable)
    sem_seg_heads_registry.register(pix)
    transformer_decoder_registry.register(dec)
    if default:
        _registered = True
    return pix, dec


def registered():
    """True when the import of this module found detectron2 + mask2former and registered the classes there."""
    return _registered


register()

VIDEO_TRANSFORMER_DECODER_NAME = "VideoMultiScaleMaskedTransformerDecoder"


def make_video_class(configurable=None):
    """The registrable subclass of video_decoder.VideoMultiScaleMaskedTransformerDecoder, under the reference's own name."""
    from . import video_decoder as _V
    deco = configurable or _configurable

    class VideoDecoderHIP(_V.VideoMultiScaleMaskedTransformerDecoder):
        @deco
        def __init__(self, *a, **k):
            super().__init__(*a, **k)

    VideoDecoderHIP.__name__ = VideoDecoderHIP.__qualname__ = VIDEO_TRANSFORMER_DECODER_NAME
    return VideoDecoderHIP


def register_video(transformer_decoder_registry=None, configurable=None):
    """Register the native clip decoder under the reference's name ``VideoMultiScaleMaskedTransformerDecoder``
    (video_mask2former_transformer_decoder.py:208), so that a video config selects it without an override.  Without a registry:
    mask2former's ``TRANSFORMER_DECODER_REGISTRY`` (returns False, registering nothing, when detectron2 or mask2former is
    missing); a registry that already holds the name — ``mask2former_video`` was imported first — refuses the second
    registration as detectron2's ``Registry`` does, and ``install_native_video_decoder`` is then the way in.  With a registry: any
    object with detectron2's ``Registry`` interface.  Returns the class (truthy) on success.  Independent of ``register()``; the
    registered decoder composes with ``install_native_video_inference`` / ``install_native_video_training``, which replace other
    parts of the model."""
    if transformer_decoder_registry is None:
        try:
            from detectron2.config import configurable as d2_configurable
            from mask2former.modeling.transformer_decoder.maskformer_transformer_decoder import TRANSFORMER_DECODER_REGISTRY
        except ImportError:
            return False
        transformer_decoder_registry = TRANSFORMER_DECODER_REGISTRY
        configurable = configurable or d2_configurable
    cls = make_video_class(configurable)
    transformer_decoder_registry.register(cls)
    return cls


SWIN_BACKBONE_NAME = "D2SwinTransformerHIP"


class _ShapeSpec:
    """channels and stride of an output map, where detectron2's ShapeSpec is not at hand"""

    def __init__(self, channels=None, height=None, width=None, stride=None):
        self.channels, self.height, self.width, self.stride = channels, height, width, stride


def make_backbone_class(backbone_base=None, shape_spec=None):
    """``D2SwinTransformerHIP``: swin.SwinTransformer built from ``cfg.MODEL.SWIN.*`` as the reference's D2SwinTransformer is
    (mask2former/modeling/backbone/swin.py:688-741), with ``output_shape()`` and ``size_divisibility``.  backbone_base:
    detectron2's ``Backbone`` (a second base class, so that detectron2 accepts the instance); shape_spec: its ``ShapeSpec``."""
    from . import swin as _S
    spec = shape_spec or _ShapeSpec
    bases = (_S.SwinTransformer,) + ((backbone_base,) if backbone_base is not None else ())

    class D2SwinTransformerHIP(*bases):
        def __init__(self, cfg, input_shape=None):
            c = cfg.MODEL.SWIN
            super().__init__(c.PRETRAIN_IMG_SIZE, c.PATCH_SIZE, 3, c.EMBED_DIM, c.DEPTHS, c.NUM_HEADS, c.WINDOW_SIZE, c.MLP_RATIO,
                             c.QKV_BIAS, c.QK_SCALE, c.DROP_RATE, c.ATTN_DROP_RATE, c.DROP_PATH_RATE, _S.nn.LayerNorm, c.APE,
                             c.PATCH_NORM, use_checkpoint=c.USE_CHECKPOINT)
            self._out_features = list(c.OUT_FEATURES)
            self._out_feature_strides = {f"res{i + 2}": 4 * 2 ** i for i in range(4)}
            self._out_feature_channels = {f"res{i + 2}": self.num_features[i] for i in range(4)}

        def forward(self, x):
            assert x.dim() == 4, f"SwinTransformer takes an input of shape (N, C, H, W). Got {x.shape} instead!"
            y = super().forward(x)
            return {k: v for k, v in y.items() if k in self._out_features}

        def output_shape(self):
            return {n: spec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}

        @property
        def size_divisibility(self):
            return 32

    D2SwinTransformerHIP.__name__ = D2SwinTransformerHIP.__qualname__ = SWIN_BACKBONE_NAME
    return D2SwinTransformerHIP


def register_backbone(backbone_registry=None, backbone_base=None, shape_spec=None):
    """Register ``D2SwinTransformerHIP`` — selected by ``MODEL.BACKBONE.NAME D2SwinTransformerHIP``.  Without a registry:
    detectron2's ``BACKBONE_REGISTRY``, ``Backbone`` and ``ShapeSpec`` (returns False, registering nothing, when detectron2 is
    missing).  With a registry: any object with detectron2's ``Registry`` interface.  Returns the class (truthy) on success.
    Independent of ``register()`` and ``register_video()``."""
    if backbone_registry is None:
        try:
            from detectron2.layers import ShapeSpec
            from detectron2.modeling import BACKBONE_REGISTRY, Backbone
        except ImportError:
            return False
        backbone_registry, backbone_base, shape_spec = BACKBONE_REGISTRY, backbone_base or Backbone, shape_spec or ShapeSpec
    cls = make_backbone_class(backbone_base, shape_spec)
    backbone_registry.register(cls)
    return cls


register_backbone()     # (as register(): at import, a no-op without detectron2)


def install_native_video_decoder(model, factored_masks=False):
    """Replace ``model.sem_seg_head.predictor`` of a reference ``VideoMaskFormer`` — its torch
    ``VideoMultiScaleMaskedTransformerDecoder`` — by the native module (video_decoder.py) built from the old one's fields, with
    the old one's state dict loaded strictly, on its device and in its training mode.  Returns the new module.  Composes with
    ``install_native_video_inference`` and ``install_native_video_training`` in any order: those replace the eval branch of
    ``forward`` and the criterion, this the module between the pixel decoder and them.
    ``factored_masks``: in training the module hands ``pred_masks`` over as ``mask_fused.FactoredClipMasks`` and never writes the
    [B, L * Q, T, h, w] maps.  Only the criterion of ``install_native_video_training`` reads that form: install both."""
    from .video_decoder import VideoMultiScaleMaskedTransformerDecoder
    old = model.sem_seg_head.predictor
    hidden = old.decoder_norm.normalized_shape[0]
    proj = [m for m in old.input_proj if hasattr(m, "weight")]
    new = VideoMultiScaleMaskedTransformerDecoder(
        in_channels=proj[0].weight.shape[1] if proj else hidden, mask_classification=old.mask_classification,
        num_classes=old.class_embed.out_features - 1, hidden_dim=hidden, num_queries=old.num_queries, nheads=old.num_heads,
        dim_feedforward=old.transformer_ffn_layers[0].linear1.out_features, dec_layers=old.num_layers,
        pre_norm=bool(old.transformer_ffn_layers[0].normalize_before), mask_dim=old.mask_embed.layers[-1].out_features,
        enforce_input_project=bool(proj), num_frames=old.num_frames)
    new.to(old.decoder_norm.weight.device)
    new.load_state_dict(old.state_dict(), strict=True)
    new.train(old.training)
    new.factored_masks = bool(factored_masks)
    model.sem_seg_head.predictor = new
    return new


def native_eval_forward(model, batched_inputs, cfg, image_list_cls=None, instance_bits=False):
    """The eval branch of a reference ``MaskFormer`` (mask2former/maskformer_model.py:199-203 + 233-279) with the native
    post-processing (inference.postprocess) in place of its F.interpolate / sem_seg_postprocess / *_inference body.
    ``instance_bits``: ``[{"instances": d}]`` with d the per-image dict of inference.instance_bits (packed masks, for
    ``InstanceAPEvaluator``) instead of the ``postprocess`` results."""
    from .inference import postprocess
    if image_list_cls is None:
        from detectron2.structures import ImageList as image_list_cls
    images = [x["image"].to(model.device) for x in batched_inputs]
    images = [(x - model.pixel_mean) / model.pixel_std for x in images]
    images = image_list_cls.from_tensors(images, model.size_divisibility)
    outputs = model.sem_seg_head(model.backbone(images.tensor))
    out_sizes = [(x.get("height", s[0]), x.get("width", s[1])) for x, s in zip(batched_inputs, images.image_sizes)]
    if instance_bits:
        from .inference import instance_bits as bits_route
        return [{"instances": d} for d in bits_route(outputs["pred_logits"], outputs["pred_masks"], images.image_sizes,
                                                     tuple(images.tensor.shape[-2:]), out_sizes, cfg)]
    return postprocess(outputs["pred_logits"], outputs["pred_masks"], images.image_sizes, tuple(images.tensor.shape[-2:]), out_sizes,
                       cfg)


def install_native_inference(model, image_list_cls=None, semantic_labels=False, instance_masks="dense", instance_bits=False,
                             instance_boxes=False):
    """Route the eval branch of a reference ``MaskFormer`` instance through ``native_eval_forward``; training is unchanged.
    ``semantic_labels`` / ``instance_masks`` / ``instance_boxes``: the evaluation-form results of inference.InferenceConfig (the
    model has no such attributes; the defaults give the reference's own result dicts, ``pred_boxes`` zeros among them).
    ``instance_bits``: the model returns only "instances", as packed masks (inference.instance_bits), the form
    ``InstanceAPEvaluator`` consumes without a dense mask.  Returns the inference.InferenceConfig in use."""
    import dataclasses
    from .inference import InferenceConfig
    cfg = dataclasses.replace(InferenceConfig.from_maskformer(model), semantic_labels=semantic_labels, instance_masks=instance_masks,
                              instance_boxes=bool(instance_boxes))
    train_forward = model.forward

    def forward(batched_inputs):
        if model.training:
            return train_forward(batched_inputs)
        return native_eval_forward(model, batched_inputs, cfg, image_list_cls, instance_bits)

    model.forward = forward
    return cfg


def native_video_eval_forward(model, batched_inputs, cfg, image_list_cls=None):
    """The eval branch of a reference ``VideoMaskFormer`` (mask2former_video/video_maskformer_model.py:180-188 + 204-225) with
    inference.postprocess_video in place of its F.interpolate of all queries and ``inference_video``: the frames of the one video
    normalised and padded together, ``backbone`` and ``sem_seg_head`` as they are, then the clip ``pred_logits[0]`` /
    ``pred_masks[0]``.  ``cfg``: an inference.VideoInferenceConfig.  Returns the ``video_output`` dict in the form ``cfg.masks``."""
    from .inference import postprocess_video
    if image_list_cls is None:
        from detectron2.structures import ImageList as image_list_cls
    if len(batched_inputs) != 1:
        raise ValueError(f"the video eval branch takes one video at a time (:208, :219), got {len(batched_inputs)}")
    images = [frame.to(model.device) for video in batched_inputs for frame in video["image"]]
    images = [(x - model.pixel_mean) / model.pixel_std for x in images]
    images = image_list_cls.from_tensors(images, model.size_divisibility)
    outputs = model.sem_seg_head(model.backbone(images.tensor))
    image_size = images.image_sizes[0]
    inp = batched_inputs[0]
    out_size = (inp.get("height", image_size[0]), inp.get("width", image_size[1]))
    return postprocess_video(outputs["pred_logits"][0], outputs["pred_masks"][0], image_size, tuple(images.tensor.shape[-2:]), out_size, cfg)


def install_native_video_inference(model, masks="dense", image_list_cls=None):
    """Route the eval branch of a reference ``VideoMaskFormer`` instance through ``native_video_eval_forward``; training is
    unchanged.  ``masks``: "dense" (the reference's result, the masks one bool tensor on the device), "bits" (packed, for
    ``YTVISEvaluatorHIP.process``) or "rle" (for ``YTVISEvaluatorHIP.results_json``).  Returns the inference.VideoInferenceConfig in
    use."""
    from .inference import VideoInferenceConfig
    cfg = VideoInferenceConfig.from_video_maskformer(model, masks=masks)
    train_forward = model.forward

    def forward(batched_inputs):
        if model.training:
            return train_forward(batched_inputs)
        return native_video_eval_forward(model, batched_inputs, cfg, image_list_cls)

    model.forward = forward
    return cfg


def install_native_video_training(model):
    """Give a reference ``VideoMaskFormer`` instance the native losses of a clip (video_losses.py): ``model.criterion`` becomes a
    ``VideoSetCriterion`` built from the old one's fields (matcher weights and points, ``num_classes``, ``weight_dict``,
    ``eos_coef``, ``losses`` and the three sampling parameters) and ``model.prepare_targets`` one that calls
    ``prepare_video_targets`` (bool masks, no float copy).  The training branch of ``forward`` (:190-203) runs on as it is; the
    eval branch and ``install_native_video_inference`` are not touched.  The criterion takes ``pred_masks`` as tensors or as
    the factors of ``install_native_video_decoder(model, factored_masks=True)``.  Returns the new criterion."""
    from .video_losses import VideoHungarianMatcher, VideoSetCriterion, prepare_video_targets
    old = model.criterion
    matcher = VideoHungarianMatcher(cost_class=old.matcher.cost_class, cost_mask=old.matcher.cost_mask,
                                    cost_dice=old.matcher.cost_dice, num_points=old.matcher.num_points)
    criterion = VideoSetCriterion(old.num_classes, matcher=matcher, weight_dict=old.weight_dict, eos_coef=old.eos_coef,
                                  losses=old.losses, num_points=old.num_points, oversample_ratio=old.oversample_ratio,
                                  importance_sample_ratio=old.importance_sample_ratio)
    criterion.to(old.empty_weight.device)
    criterion.train(getattr(old, "training", True))

    def prepare_targets(targets, images):
        padded_hw = tuple(images.tensor.shape[-2:])
        out = []
        for video in targets:
            frames = [fr.to(model.device) for fr in video["instances"]]
            out.append(prepare_video_targets([fr.gt_masks.tensor for fr in frames], [fr.gt_ids for fr in frames],
                                             frames[-1].gt_classes, padded_hw))
        return out

    model.criterion = criterion
    model.prepare_targets = prepare_targets
    return criterion


class YTVISEvaluatorHIP:
    """The reference's ``YTVISEvaluator`` (mask2former_video/data_video/ytvis_eval.py) where the ground truth is at hand, on
    inference.TubeAP: tubes are matched on the device, one record per detection crosses to the host at ``evaluate``.  Needs neither
    detectron2 nor pycocotools.

    ``process(inputs, outputs)``: ``outputs`` the "bits" form of inference.postprocess_video (one video), ``inputs[0]["instances"]``
    the video's ground-truth tubes: ``gt_masks`` dense [G, F, H, W] (any of ``pack_masks``' dtypes; a frame without annotation all
    zero) or packed int64 [G, F, nwords], ``gt_classes`` [G], optional ``gt_iscrowd`` [G].
    ``evaluate()`` -> {"segm": {AP, AP50, AP75, APs, APm, APl, AR1, AR10, AP-{name}...}} (ytvis_eval.py:205).
    In place of ``gt_masks`` the ground truth may carry ``"segmentations"``, [G][F] entries as a YouTube-VIS json holds them
    (``None`` for a frame without annotation, an RLE dict with a list or a string, or a polygon list) at the prediction's size:
    inference.segmentation_bits decodes them on the device, no dense mask exists on the host.
    ``results_json(video_id, output, compressed=False)``: the submission entries of ``instances_to_coco_json_video`` (:256-293)
    from the "rle" form.  Their "counts" are uncompressed run lengths (column-major, starting with the zeros);
    ``compressed=True`` makes them the COCO strings a submission file holds (inference.rle_compress, pycocotools' ``frPyObjects``).
    The image route's ``pred_masks_rle`` go through ``compress_rles`` of this module."""

    def __init__(self, num_classes, class_names=None, device="cuda:0", **ap_options):
        from .inference import TubeAP
        self.ap = TubeAP(num_classes, device=device, **ap_options)
        if class_names is not None and len(class_names) != self.ap.num_classes:
            raise ValueError(f"{len(class_names)} class names for {self.ap.num_classes} classes")
        self.class_names = class_names

    def reset(self):
        self.ap.reset()

    def process(self, inputs, outputs):
        import torch
        from .inference import pack_masks
        if len(inputs) != 1:
            raise ValueError("More than one inputs are loaded for inference!")      # ytvis_eval.py:267
        if "bits" not in outputs:
            raise ValueError("YTVISEvaluatorHIP.process takes the 'bits' form of postprocess_video (install_native_video_inference("
                             "model, masks='bits'))")
        dev = self.ap.device
        dt_bits = outputs["bits"]
        F, nwords = dt_bits.shape[1:]
        H, W = outputs["size"]
        gt = inputs[0]["instances"]
        segs = gt.get("segmentations") if isinstance(gt, dict) and "gt_masks" not in gt else None
        if segs is not None:                                 # as the json holds them: decoded on the device, never dense on the host
            from .inference import segmentation_bits
            G = len(segs)
            if any(len(tube) != F for tube in segs):
                raise ValueError(f"segmentations must be [G][{F}], one entry (or None) per frame of the prediction")
            gm = None
            gt_bits = segmentation_bits([s for tube in segs for s in tube], (H, W), device=dev).view(G, F, nwords)
        else:
            gm = gt["gt_masks"]
            gm = getattr(gm, "tensor", gm).to(dev)
            G = gm.shape[0]
        if gm is None:
            pass
        elif G == 0:
            gt_bits = dt_bits.new_empty((0, F, nwords))
        elif gm.dim() == 4:
            if tuple(gm.shape[1:]) != (F, H, W):
                raise ValueError(f"gt_masks {tuple(gm.shape)} are not [G, {F}, {H}, {W}], the prediction's frames and size")
            gt_bits = pack_masks(gm.reshape(G * F, H, W)).view(G, F, nwords)
        else:
            gt_bits = gm
        crowd = gt.get("gt_iscrowd")
        self.ap.update(dt_bits, outputs["pred_scores"], outputs["pred_labels"], gt_bits, gt["gt_classes"],
                       torch.zeros(G, dtype=torch.int32) if crowd is None else crowd, dt_frame_area=outputs["frame_area"])

    def evaluate(self):
        return {"segm": self.ap.results(self.class_names)}

    @staticmethod
    def results_json(video_id, output, compressed=False):
        if "pred_masks_rle" not in output:
            raise ValueError("YTVISEvaluatorHIP.results_json takes the 'rle' form of postprocess_video")
        tubes = [compress_rles(segms) for segms in output["pred_masks_rle"]] if compressed else output["pred_masks_rle"]
        return [{"video_id": video_id, "score": s, "category_id": l, "segmentations": segms}
                for s, l, segms in zip(output["pred_scores"], output["pred_labels"], tubes)]


def compress_rles(rles):
    """Uncompressed RLE dicts (the image route's ``pred_masks_rle``, a tube of the video route's, ``inference.bits_rle``) -> the
    dicts a COCO results json holds, "counts" the compressed string (inference.rle_compress); a ``None`` entry stays ``None``."""
    from .inference import rle_compress
    return [None if r is None else rle_compress(r) for r in rles]


def is_hflip(tfm):
    """True when any transform of a ``TransformList`` (or a bare list of transforms) is an ``HFlipTransform``
    (test_time_augmentation.py:87): by ``isinstance`` where fvcore is importable, else by class name."""
    tfms = getattr(tfm, "transforms", tfm)
    try:
        from fvcore.transforms import HFlipTransform
    except ImportError:
        return any(type(t).__name__ == "HFlipTransform" for t in tfms)
    return any(isinstance(t, HFlipTransform) for t in tfms)


class SemanticSegmentorWithTTAHIP:
    """The reference's ``SemanticSegmentorWithTTA`` (mask2former/test_time_augmentation.py:21-103) on inference.SemanticTTA:
    ``__call__(batched_inputs)`` -> one ``{"sem_seg"}`` dict per input (``{"sem_seg_labels"}`` with ``semantic_labels``), the
    mean over the augmented views of ``tta_mapper(input)``, flipped views mirrored back.  Each view runs through
    ``model.backbone`` / ``model.sem_seg_head`` as in ``native_eval_forward``, one view at a time as in the reference
    (``batch_size`` is accepted and unused there too).  With ``sem_seg_postprocess_before_inference`` no per-view scores exist;
    in the other mode one view's ``[K, hi, wi]`` scores at a time live in native scratch, which is sized by the largest view
    and kept between images."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=1, *, image_list_cls=None, semantic_labels=False):
        import dataclasses
        from .inference import InferenceConfig
        model = getattr(model, "module", model) if type(model).__name__ == "DistributedDataParallel" else model
        if tta_mapper is None:
            try:
                from detectron2.modeling import DatasetMapperTTA
            except ImportError as e:
                raise ImportError("SemanticSegmentorWithTTAHIP: tta_mapper=None builds detectron2.modeling.DatasetMapperTTA(cfg), and "
                                  "detectron2 is not importable; pass a tta_mapper (input dict -> list of augmented dicts with "
                                  "'image' and 'transforms')") from e
            tta_mapper = DatasetMapperTTA(cfg)
        self.cfg = cfg.clone() if hasattr(cfg, "clone") else cfg
        self.model = model
        self.tta_mapper = tta_mapper
        self.batch_size = batch_size
        self.image_list_cls = image_list_cls
        self.inference_cfg = dataclasses.replace(InferenceConfig.from_maskformer(model), semantic_labels=semantic_labels)
        if not self.inference_cfg.semantic_on:
            raise ValueError("SemanticSegmentorWithTTAHIP needs a model with semantic_on")

    def _prepared(self, x):
        """A copy of one input dict that has what a view needs: the "image" as a CHW tensor (decoded in the model's input format
        where only "file_name" came) and the output size, which defaults to the image's own."""
        x = dict(x)
        if "image" not in x:
            import torch
            from detectron2.data.detection_utils import read_image
            hwc = read_image(x.pop("file_name"), format=self.model.input_format)
            x["image"] = torch.as_tensor(hwc.copy()).permute(2, 0, 1).contiguous()
        x.setdefault("height", int(x["image"].shape[-2]))
        x.setdefault("width", int(x["image"].shape[-1]))
        return x

    def __call__(self, batched_inputs):
        return [self._inference_one_image(self._prepared(x)) for x in batched_inputs]

    def _inference_one_image(self, inp):
        import torch
        from .inference import SemanticTTA
        image_list_cls = self.image_list_cls
        if image_list_cls is None:
            from detectron2.structures import ImageList as image_list_cls
        model = self.model
        out_size = (int(inp["height"]), int(inp["width"]))
        tta = SemanticTTA(self.inference_cfg)
        with torch.no_grad():
            for view in self.tta_mapper(inp):
                image = (view["image"].to(model.device) - model.pixel_mean) / model.pixel_std
                images = image_list_cls.from_tensors([image], model.size_divisibility)
                outputs = model.sem_seg_head(model.backbone(images.tensor))
                tta.add(outputs["pred_logits"], outputs["pred_masks"], images.image_sizes[0], tuple(images.tensor.shape[-2:]), out_size,
                        is_hflip(view["transforms"]))
            return tta.result()


def _read_png_rgb(path):
    """The panoptic PNG as uint8 [H, W, 3] (R, G, B), through PIL."""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class PanopticQualityEvaluator:
    """detectron2's evaluator protocol (``reset`` / ``process(inputs, outputs)`` / ``evaluate``) on inference.PanopticQuality, in
    place of ``COCOPanopticEvaluator``: the predicted id map stays on the device, the ground-truth PNG goes up as its RGB bytes
    (3 bytes per pixel) and is decoded by the kernel.  Writes no file and needs neither detectron2 nor panopticapi.

    ``dataset_id_to_contiguous_id``: the union of the metadata's thing_ and stuff_dataset_id_to_contiguous_id, applied to the
    ground truth's category ids (the model's are contiguous already).  ``read_png``: path -> uint8 [H, W, 3]."""

    def __init__(self, num_classes, thing_ids, dataset_id_to_contiguous_id, read_png=None, void_id=0, device="cuda:0"):
        from .inference import PanopticQuality
        self.id_map = {int(k): int(v) for k, v in dict(dataset_id_to_contiguous_id).items()}
        self.read_png = read_png or _read_png_rgb
        self.pq = PanopticQuality(num_classes, thing_ids, void_id=void_id, device=device)

    def reset(self):
        self.pq.reset()

    def gt_segments(self, segments_info):
        """The annotation's segments with contiguous category ids, in the annotation's order."""
        out = []
        for s in segments_info:
            c = int(s["category_id"])
            if c not in self.id_map:
                raise ValueError(f"ground-truth segment {s['id']} has category_id {c}, which the dataset mapping does not list")
            out.append({"id": int(s["id"]), "category_id": self.id_map[c], "iscrowd": int(s.get("iscrowd", 0))})
        return out

    def process(self, inputs, outputs):
        import numpy as np
        from . import _h2d
        for inp, out in zip(inputs, outputs):
            ids, segments_info = out["panoptic_seg"]
            rgb = np.ascontiguousarray(self.read_png(inp["pan_seg_file_name"]), dtype=np.uint8)
            gt = _h2d.upload(rgb, self.pq.device)
            self.pq.update(ids, segments_info, gt, self.gt_segments(inp["segments_info"]))

    def evaluate(self):
        return {"panoptic_seg": self.pq.results()}


class InstanceAPEvaluator:
    """detectron2's evaluator protocol (``reset`` / ``process(inputs, outputs)`` / ``evaluate``) on inference.InstanceAP, in place
    of ``COCOEvaluator`` for "segm" and of the reference's tools/evaluate_coco_boundary_ap.py (boundary-iou-api) for "boundary":
    masks are packed and matched on the device, one record per detection and score crosses to the host at ``evaluate``.  Writes no
    file and needs neither detectron2, pycocotools nor boundary_iou.

    iou_types: any of "segm", "boundary", "bbox"; one ``InstanceAP`` per type (``self.aps``), the masks of an image packed once and
    their pair intersections counted once for all of them.  ``evaluate`` returns one key per type.  "bbox" (COCOEvaluator's task of
    that name) takes the detections' boxes from ``"boxes"`` (inference.instance_bits with ``instance_boxes``) or ``pred_boxes``
    where the prediction carries them, the ground truth's from ``gt_boxes`` (a tensor or an object with ``.tensor``), all XYXY; a
    side without boxes gets those of its masks (inference.mask_boxes).  ``pred_boxes`` of a model installed without
    ``instance_boxes`` are the reference's placeholder, all zero on the host: they count as absent and the masks' boxes are scored.

    Predictions: ``outputs[i]["instances"]`` with dense ``pred_masks`` [T, H, W], ``scores`` and ``pred_classes`` (packed here), or
    the dict of inference.instance_bits where the model was installed with ``install_native_inference(..., instance_bits=True)``.
    Ground truth: ``inputs[i]["instances"]`` with ``gt_masks`` (a [G, H, W] tensor or an object with ``.tensor``) and ``gt_classes``
    at the prediction's size; optional ``gt_iscrowd`` and ``gt_areas`` (missing: no crowd, the pixel counts).
    An input without ``"instances"`` may carry ``"annotations"`` instead, the COCO dicts of the image as the json holds them
    (``segmentation`` as polygons, RLE or compressed RLE at the prediction's size, ``category_id``, optional ``iscrowd``, ``area``,
    ``bbox``): inference.segmentation_bits decodes them on the device, ``area`` / ``bbox`` (XYWH) are used where every annotation of
    the image has them, and ``dataset_id_to_contiguous`` (a dict; None: identity) maps the category ids."""

    def __init__(self, num_classes, class_names=None, device="cuda:0", iou_types=("segm",), dilation_ratio=0.02,
                 dataset_id_to_contiguous=None, **ap_options):
        from .inference import InstanceAP
        self.dataset_id_to_contiguous = None if dataset_id_to_contiguous is None else dict(dataset_id_to_contiguous)
        iou_types = tuple(iou_types)
        if not iou_types or len(set(iou_types)) != len(iou_types):
            raise ValueError(f"iou_types must list each wanted type once, got {iou_types!r}")
        self.aps = {t: InstanceAP(num_classes, device=device, iou_type=t, dilation_ratio=dilation_ratio, **ap_options) for t in iou_types}
        self.ap = self.aps[iou_types[0]]
        if class_names is not None and len(class_names) != self.ap.num_classes:
            raise ValueError(f"{len(class_names)} class names for {self.ap.num_classes} classes")
        self.class_names = class_names

    def reset(self):
        for ap in self.aps.values():
            ap.reset()

    @staticmethod
    def _field(inst, name, default=None):
        if isinstance(inst, dict):
            return inst.get(name, default)
        if hasattr(inst, "has") and not inst.has(name):
            return default
        return getattr(inst, name, default)

    def _xywh(self, boxes, placeholder_is_absent=False):
        """XYXY boxes (a tensor or an object with ``.tensor``) -> XYWH float64 on the evaluator's device; None stays None.
        ``placeholder_is_absent``: host boxes that are all zero are the reference's placeholder (``Boxes(torch.zeros(T, 4))``, what
        a model installed without ``instance_boxes`` returns), not boxes: None, so that the masks' boxes are scored.  Only host
        tensors are looked at: reading a device tensor here would stall the loop, and real boxes are not all zero."""
        from .inference import boxes_xyxy_to_xywh
        if boxes is None:
            return None
        boxes = getattr(boxes, "tensor", boxes)
        if placeholder_is_absent and not boxes.is_cuda and not bool(boxes.any()):
            return None
        return boxes_xyxy_to_xywh(boxes.to(self.ap.device))

    def process(self, inputs, outputs):
        import torch
        from .inference import pack_masks
        dev = self.ap.device
        for inp, out in zip(inputs, outputs):
            pred = out["instances"]
            if isinstance(pred, dict) and "bits" in pred:
                dt_bits, size = pred["bits"], tuple(pred["size"])
            else:
                masks = self._field(pred, "pred_masks")
                dt_bits, size = pack_masks(masks.to(dev)), tuple(masks.shape[-2:])
            if "instances" not in inp and "annotations" in inp:
                args, gt_boxes = self._annotation_args(inp["annotations"], size)
                self._update(pred, (dt_bits, self._field(pred, "scores"), self._field(pred, "pred_classes")) + args, size, gt_boxes)
                continue
            gt = inp["instances"]
            gm = self._field(gt, "gt_masks")
            gm = getattr(gm, "tensor", gm)
            if gm.shape[0] == 0:                             # an image without annotations, whatever shape its empty tensor has
                gm = gm.new_zeros((0,) + size)
            elif gm.dim() != 3 or tuple(gm.shape[-2:]) != size:
                raise ValueError(f"gt_masks {tuple(gm.shape)} do not have the prediction's size {size}")
            G = gm.shape[0]
            crowd = self._field(gt, "gt_iscrowd")
            args = (dt_bits, self._field(pred, "scores"), self._field(pred, "pred_classes"), pack_masks(gm.to(dev)),
                    self._field(gt, "gt_classes"), torch.zeros(G, dtype=torch.int32) if crowd is None else crowd,
                    self._field(gt, "gt_areas"))
            self._update(pred, args, size, self._xywh(self._field(gt, "gt_boxes")))

    def _update(self, pred, args, size, gt_boxes):
        """one image into every type's InstanceAP: args as ``InstanceAP.update`` takes them, gt_boxes XYWH or None"""
        from .inference import mask_pair_counts
        counts = None
        for t, ap in self.aps.items():
            if t == "bbox":
                dt_boxes = self._xywh(self._field(pred, "boxes", self._field(pred, "pred_boxes")), placeholder_is_absent=True)
                ap.update(*args, size=size, dt_boxes=dt_boxes, gt_boxes=gt_boxes)
                continue
            if counts is None:
                counts = mask_pair_counts(args[0], args[3])      # once for every type that counts pixels
            ap.update(*args, size=size, pair_counts=counts)

    def _annotation_args(self, annotations, size):
        """COCO annotation dicts of one image -> the ground-truth arguments of ``InstanceAP.update`` (bits, classes, crowd, areas) and
        the XYWH boxes: the segmentations decoded on the device at the prediction's size, "area" / "bbox" used where EVERY annotation
        has them (else the pixel counts / the masks' boxes), "category_id" mapped through ``dataset_id_to_contiguous``."""
        import torch
        from .inference import segmentation_bits
        dev = self.ap.device
        ids = self.dataset_id_to_contiguous
        for a in annotations:
            if ids is not None and a["category_id"] not in ids:
                raise ValueError(f"category_id {a['category_id']} is not in dataset_id_to_contiguous")
        classes = torch.tensor([a["category_id"] if ids is None else ids[a["category_id"]] for a in annotations], dtype=torch.int64)
        crowd = torch.tensor([int(a.get("iscrowd", 0)) for a in annotations], dtype=torch.int32)
        G = len(annotations)
        areas = torch.tensor([float(a["area"]) for a in annotations], dtype=torch.float64) \
            if G and all("area" in a for a in annotations) else None
        boxes = torch.tensor([[float(v) for v in a["bbox"]] for a in annotations], dtype=torch.float64).reshape(G, 4).to(dev) \
            if G and all("bbox" in a for a in annotations) else None
        bits = segmentation_bits([a["segmentation"] for a in annotations], size, device=dev)
        return (bits, classes, crowd, areas), boxes

    def evaluate(self):
        return {t: ap.results(self.class_names) for t, ap in self.aps.items()}


def _read_image_default():
    """detectron2's ``detection_utils.read_image`` where importable, else PIL's decode to RGB (BGR on request)"""
    try:
        from detectron2.data.detection_utils import read_image
        return read_image
    except ImportError:
        def read_image(file_name, format=None):
            import numpy as np
            from PIL import Image
            with Image.open(file_name) as im:
                a = np.asarray(im.convert("RGB"))
            return a[:, :, ::-1] if format == "BGR" else a
        return read_image


class COCOInstanceLSJDeviceMapper:
    """The worker side of the reference's ``COCOInstanceNewBaselineDatasetMapper``
    (mask2former/data/dataset_mappers/coco_instance_new_baseline_dataset_mapper.py) when large-scale jitter runs on the device
    (augment.py): it reads the image, DRAWS the geometry (flip, scale, crop, in the reference's order from ``numpy.random``) and
    returns the dict with ``"image_raw"`` (uint8 [H, W, 3]), ``"lsj"`` (``augment.LSJParams``) and the non-crowd ``"annotations"``
    without keypoints.  No resize and no rasterisation on the worker: ``install_native_lsj`` forms the batch on the model's device.
    ``cls(cfg, is_train)`` reads ``cfg.INPUT`` as the reference's ``from_config`` does."""

    @_configurable
    def __init__(self, is_train=True, *, image_size, min_scale, max_scale, random_flip, image_format, read_image=None):
        if not is_train:
            raise ValueError("COCOInstanceLSJDeviceMapper: only training augmentation, as the reference's build_transform_gen")
        if random_flip not in ("horizontal", "none"):
            raise ValueError(f"COCOInstanceLSJDeviceMapper: random_flip must be 'horizontal' or 'none', got {random_flip!r}")
        self.is_train, self.image_size, self.min_scale, self.max_scale = bool(is_train), image_size, float(min_scale), float(max_scale)
        self.random_flip, self.image_format = random_flip, image_format
        self.read_image = read_image or _read_image_default()

    @classmethod
    def from_config(cls, cfg, is_train=True):
        return {"is_train": is_train, "image_size": cfg.INPUT.IMAGE_SIZE, "min_scale": cfg.INPUT.MIN_SCALE,
                "max_scale": cfg.INPUT.MAX_SCALE, "random_flip": cfg.INPUT.RANDOM_FLIP, "image_format": cfg.INPUT.FORMAT}

    def __call__(self, dataset_dict):
        import numpy as np
        import torch
        from .augment import draw_lsj
        d = {k: v for k, v in dataset_dict.items() if k != "annotations"}
        image = np.ascontiguousarray(self.read_image(dataset_dict["file_name"], format=self.image_format))
        if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
            raise ValueError(f"COCOInstanceLSJDeviceMapper: expected a uint8 [H, W, 3] image, got {image.dtype} {image.shape}")
        for key, n in (("height", image.shape[0]), ("width", image.shape[1])):
            if key in d and d[key] != n:
                raise ValueError(f"COCOInstanceLSJDeviceMapper: {dataset_dict['file_name']} has {key} {n}, the dataset says {d[key]}")
        d["image_raw"] = torch.from_numpy(image)
        d["lsj"] = draw_lsj(image.shape[0], image.shape[1], image_size=self.image_size, min_scale=self.min_scale,
                            max_scale=self.max_scale, flip=self.random_flip == "horizontal", rng=np.random)
        if "annotations" in dataset_dict:
            d["annotations"] = [{k: v for k, v in a.items() if k != "keypoints"} for a in dataset_dict["annotations"]
                                if a.get("iscrowd", 0) == 0]
        return d


def native_lsj_inputs(batched_inputs, device):
    """The dicts of ``COCOInstanceLSJDeviceMapper`` -> copies with ``"image"`` (uint8 [3, S, S] on ``device``) and ``"instances"``
    (``gt_classes``, ``gt_masks`` bool [T, S, S], ``gt_boxes``, ``image_size``), as the reference's mapper would have left them: one
    resample launch and one polygon pass for the batch (augment.lsj_batch)."""
    from .augment import lsj_batch
    from .inference import _structures
    Boxes, Instances = _structures()
    images, targets = lsj_batch(batched_inputs, device=device)
    out = []
    for x, image, t in zip(batched_inputs, images, targets):
        p = x["lsj"]
        d = {k: v for k, v in x.items() if k not in ("image_raw", "annotations")}
        d["image"] = image[:, :p.crop[0], :p.crop[1]]
        inst = Instances(tuple(p.crop))
        inst.gt_classes = t["labels"]
        inst.gt_masks = t["masks"]
        inst.gt_boxes = Boxes(t["boxes"])
        d["instances"] = inst
        out.append(d)
    return out


def install_native_lsj(model):
    """Route the training branch of a model fed by ``COCOInstanceLSJDeviceMapper`` through ``native_lsj_inputs``: ``forward`` forms
    the batch on the model's device and hands the usual dicts ("image", "instances") on, so the model's own normalisation and
    ``prepare_targets`` run unchanged.  Eval mode is passed through untouched.  Works without detectron2 (the ``Instances``
    stand-in of inference.py)."""
    inner = model.forward

    def forward(batched_inputs):
        if not model.training:
            return inner(batched_inputs)
        return inner(native_lsj_inputs(batched_inputs, model.device))

    model.forward = forward
    return forward


# ---- panoptic and semantic training input from label maps (label_input.py) ------------------------------------------------------------
def _read_worker_image(read_image, dataset_dict, image_format, who):
    import numpy as np
    image = np.ascontiguousarray(read_image(dataset_dict["file_name"], format=image_format))
    if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
        raise ValueError(f"{who}: expected a uint8 [H, W, 3] image, got {image.dtype} {image.shape}")
    for key, n in (("height", image.shape[0]), ("width", image.shape[1])):
        if key in dataset_dict and dataset_dict[key] != n:
            raise ValueError(f"{who}: {dataset_dict['file_name']} has {key} {n}, the dataset says {dataset_dict[key]}")
    return image


def _read_label_default():
    """detectron2's ``read_image(path)`` without a format where importable (the file's own mode), else PIL's decode as it is"""
    try:
        from detectron2.data.detection_utils import read_image
        return read_image
    except ImportError:
        def read_label(file_name):
            import numpy as np
            from PIL import Image
            with Image.open(file_name) as im:
                return np.asarray(im)
        return read_label


class COCOPanopticLSJDeviceMapper:
    """The worker side of the reference's ``COCOPanopticNewBaselineDatasetMapper``
    (mask2former/data/dataset_mappers/coco_panoptic_new_baseline_dataset_mapper.py) when the augmentation runs on the device: it
    reads the image and the panoptic PNG, DRAWS the geometry as ``COCOInstanceLSJDeviceMapper`` does and returns the dict with
    ``"image_raw"`` and ``"pan_raw"`` (uint8 [H, W, 3] each), ``"lsj"`` (``augment.LSJParams``) and ``"segments_info"``.  No resize
    and no mask on the worker: two decoded images cross instead of up to a hundred dense planes."""

    @_configurable
    def __init__(self, is_train=True, *, image_size, min_scale, max_scale, random_flip, image_format, read_image=None):
        if not is_train:
            raise ValueError("COCOPanopticLSJDeviceMapper: only training augmentation, as the reference's build_transform_gen")
        if random_flip == "vertical":
            raise NotImplementedError("INPUT.RANDOM_FLIP 'vertical': only the horizontal flip is implemented on the device path")
        if random_flip not in ("horizontal", "none"):
            raise ValueError(f"COCOPanopticLSJDeviceMapper: random_flip must be 'horizontal' or 'none', got {random_flip!r}")
        self.is_train, self.image_size, self.min_scale, self.max_scale = bool(is_train), image_size, float(min_scale), float(max_scale)
        self.random_flip, self.image_format = random_flip, image_format
        self.read_image = read_image or _read_image_default()

    @classmethod
    def from_config(cls, cfg, is_train=True):
        return {"is_train": is_train, "image_size": cfg.INPUT.IMAGE_SIZE, "min_scale": cfg.INPUT.MIN_SCALE,
                "max_scale": cfg.INPUT.MAX_SCALE, "random_flip": cfg.INPUT.RANDOM_FLIP, "image_format": cfg.INPUT.FORMAT}

    def __call__(self, dataset_dict):
        import numpy as np
        import torch
        from .augment import draw_lsj
        who = "COCOPanopticLSJDeviceMapper"
        d = {k: v for k, v in dataset_dict.items() if k not in ("annotations", "pan_seg_file_name")}
        image = _read_worker_image(self.read_image, dataset_dict, self.image_format, who)
        d["image_raw"] = torch.from_numpy(image)
        d["lsj"] = draw_lsj(image.shape[0], image.shape[1], image_size=self.image_size, min_scale=self.min_scale,
                            max_scale=self.max_scale, flip=self.random_flip == "horizontal", rng=np.random)
        if "pan_seg_file_name" in dataset_dict:
            pan = np.ascontiguousarray(self.read_image(dataset_dict["pan_seg_file_name"], format="RGB"))
            if pan.dtype != np.uint8 or pan.shape != image.shape:
                raise ValueError(f"{who}: the panoptic PNG must be uint8 {image.shape}, got {pan.dtype} {pan.shape}")
            d["pan_raw"] = torch.from_numpy(pan)
            d["segments_info"] = list(dataset_dict["segments_info"])
        return d


class SemanticDeviceMapper:
    """The worker side of the reference's ``MaskFormerSemanticDatasetMapper``
    (mask2former/data/dataset_mappers/mask_former_semantic_dataset_mapper.py) when the augmentation runs on the device: it reads the
    image and the label map and DRAWS (``augment.draw_semseg``: the short edge, the crop origins, the flip) and returns the dict
    with ``"image_raw"`` (uint8 [H, W, 3]), ``"sem_seg_raw"`` (uint8 [H, W]; int32 for a map with labels above 255) and
    ``"semseg"`` (``augment.SemSegDraw``).  All ten candidate origins of ``RandomCrop_CategoryAreaConstraint`` are drawn up front,
    because the counts that decide between them are taken on the device: the windows have the reference's distribution, but its RNG
    stream is consumed differently (the reference stops drawing at the first accepted window)."""

    @_configurable
    def __init__(self, is_train=True, *, min_size, max_size, sampling, crop_enabled, crop_type, crop_size, single_category_max_area,
                 color_aug_ssd, image_format, ignore_label, size_divisibility, num_classes, read_image=None, read_label=None):
        if not is_train:
            raise ValueError("SemanticDeviceMapper: only training, as the reference's mapper asserts")
        if color_aug_ssd:
            raise NotImplementedError("INPUT.COLOR_AUG_SSD: its saturation and hue steps are OpenCV's 8-bit HSV tables, which are not "
                                      "pinned; not implemented on the device path")
        if crop_enabled and crop_type != "absolute":
            raise NotImplementedError(f"INPUT.CROP.TYPE {crop_type!r}: only 'absolute' is implemented on the device path")
        self.is_train = True
        self.min_size = (min_size,) if isinstance(min_size, int) else tuple(min_size)
        self.max_size, self.sampling = int(max_size), sampling
        self.crop = (int(crop_size[0]), int(crop_size[1])) if crop_enabled else None
        self.crop_type, self.single_category_max_area = crop_type, float(single_category_max_area)
        self.image_format, self.ignore_label, self.size_divisibility = image_format, int(ignore_label), int(size_divisibility)
        self.num_classes = int(num_classes)
        self.read_image = read_image or _read_image_default()
        self.read_label = read_label or _read_label_default()

    @classmethod
    def from_config(cls, cfg, is_train=True):
        try:
            from detectron2.data import MetadataCatalog
            ignore_label = MetadataCatalog.get(cfg.DATASETS.TRAIN[0]).ignore_label
        except ImportError:
            ignore_label = cfg.MODEL.SEM_SEG_HEAD.IGNORE_VALUE
        return {"is_train": is_train, "min_size": cfg.INPUT.MIN_SIZE_TRAIN, "max_size": cfg.INPUT.MAX_SIZE_TRAIN,
                "sampling": cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING, "crop_enabled": cfg.INPUT.CROP.ENABLED, "crop_type": cfg.INPUT.CROP.TYPE,
                "crop_size": cfg.INPUT.CROP.SIZE, "single_category_max_area": cfg.INPUT.CROP.SINGLE_CATEGORY_MAX_AREA,
                "color_aug_ssd": cfg.INPUT.COLOR_AUG_SSD, "image_format": cfg.INPUT.FORMAT, "ignore_label": ignore_label,
                "size_divisibility": cfg.INPUT.SIZE_DIVISIBILITY, "num_classes": cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES}

    def __call__(self, dataset_dict):
        import numpy as np
        import torch
        from .augment import draw_semseg
        who = "SemanticDeviceMapper"
        if "annotations" in dataset_dict:
            raise ValueError("Semantic segmentation dataset should not have 'annotations'.")
        if "sem_seg_file_name" not in dataset_dict:
            raise ValueError("Cannot find 'sem_seg_file_name' for semantic segmentation dataset {}.".format(dataset_dict["file_name"]))
        d = {k: v for k, v in dataset_dict.items() if k != "sem_seg_file_name"}
        image = _read_worker_image(self.read_image, dataset_dict, self.image_format, who)
        sem = np.asarray(self.read_label(dataset_dict["sem_seg_file_name"]))
        if sem.ndim != 2 or sem.shape != image.shape[:2] or sem.dtype.kind not in "iu":
            raise ValueError(f"{who}: the label map must be an integer {image.shape[:2]} array, got {sem.dtype} {sem.shape}")
        sem = np.ascontiguousarray(sem if sem.dtype == np.uint8 else sem.astype(np.int32))
        d["image_raw"], d["sem_seg_raw"] = torch.from_numpy(image), torch.from_numpy(sem)
        d["semseg"] = draw_semseg(image.shape[0], image.shape[1], self.min_size, self.max_size, self.sampling, crop=self.crop,
                                  crop_type=self.crop_type, single_category_max_area=self.single_category_max_area, flip=True,
                                  size_divisibility=self.size_divisibility, rng=np.random)
        return d


class MaskFormerPanopticDeviceMapper:
    """ADE20K panoptic (the reference's ``MaskFormerPanopticDatasetMapper``): a composition of the semantic geometry and the
    panoptic targets that is not built yet."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("MaskFormerPanopticDatasetMapper (ADE20K panoptic) is not implemented on the device path")


def _instances(size, t):
    from .inference import _structures
    Boxes, Instances = _structures()
    inst = Instances(tuple(size))
    inst.gt_classes = t["labels"]
    inst.gt_masks = t["masks"]
    inst.gt_boxes = Boxes(t["boxes"])
    return inst


def native_panoptic_inputs(batched_inputs, device):
    """The dicts of ``COCOPanopticLSJDeviceMapper`` -> copies with ``"image"`` (uint8 [3, S, S] on ``device``) and ``"instances"``
    (``gt_classes``, ``gt_masks`` bool [T, S, S], ``gt_boxes``), as the reference's mapper would have left them: one image launch,
    one label launch and one mask launch per image (label_input.panoptic_lsj_batch); no host wait."""
    from .label_input import panoptic_lsj_batch
    with_gt = all("pan_raw" in x for x in batched_inputs)
    if not with_gt:
        raise ValueError("native_panoptic_inputs: every input needs 'pan_raw' and 'segments_info' (a training batch)")
    images, targets = panoptic_lsj_batch(batched_inputs, device=device)
    out = []
    for x, image, t in zip(batched_inputs, images, targets):
        p = x["lsj"]
        d = {k: v for k, v in x.items() if k not in ("image_raw", "pan_raw")}
        d["image"] = image[:, :p.crop[0], :p.crop[1]]
        d["instances"] = _instances(p.crop, t)
        out.append(d)
    return out


def native_semantic_inputs(batched_inputs, device, num_classes, ignore_label, single_category_max_area=1.0):
    """The dicts of ``SemanticDeviceMapper`` -> copies with ``"image"`` (uint8 [3, Hc, Wc] on ``device``, padded to the size
    divisibility with 128), ``"sem_seg"`` (int64 [Hc, Wc], padded with the ignore label) and ``"instances"`` (one mask per class
    present), as the reference's mapper would have left them (label_input.semantic_batch: one host wait, for the window counts)."""
    from .label_input import semantic_batch
    images, targets = semantic_batch(batched_inputs, num_classes, ignore_label, single_category_max_area, device=device)
    out = []
    for x, image, t in zip(batched_inputs, images, targets):
        Hc, Wc = t["params"].canvas
        d = {k: v for k, v in x.items() if k not in ("image_raw", "sem_seg_raw")}
        d["image"] = image[:, :Hc, :Wc]
        d["sem_seg"] = t["sem_seg"]
        d["instances"] = _instances((Hc, Wc), t)
        out.append(d)
    return out


def _install_inputs(model, make):
    inner = model.forward

    def forward(batched_inputs):
        if not model.training:
            return inner(batched_inputs)
        return inner(make(batched_inputs))

    model.forward = forward
    return forward


def install_native_panoptic_lsj(model):
    """As ``install_native_lsj`` for a model fed by ``COCOPanopticLSJDeviceMapper``: the training branch gets the usual dicts
    ("image", "instances") formed on the model's device; eval mode is passed through untouched."""
    return _install_inputs(model, lambda batch: native_panoptic_inputs(batch, model.device))


def install_native_semantic_input(model, mapper=None, *, num_classes=None, ignore_label=None, single_category_max_area=None):
    """As ``install_native_lsj`` for a model fed by ``SemanticDeviceMapper``: pass the mapper (its ``num_classes``, ``ignore_label``
    and ``single_category_max_area`` are used) or the three values.  Eval mode is passed through untouched."""
    if mapper is None and (num_classes is None or ignore_label is None):
        raise ValueError("install_native_semantic_input: pass the SemanticDeviceMapper, or num_classes and ignore_label")
    K = mapper.num_classes if num_classes is None else num_classes
    ignore = mapper.ignore_label if ignore_label is None else ignore_label
    area = (mapper.single_category_max_area if mapper is not None else 1.0) if single_category_max_area is None else single_category_max_area
    return _install_inputs(model, lambda batch: native_semantic_inputs(batch, model.device, K, ignore, area))


# ---- video training input (clip_input.py) -----------------------------------------------------------------------------------------------
class YTVISClipDeviceMapper:
    """The worker side of the reference's ``YTVISDatasetMapper`` (mask2former_video/data_video/dataset_mapper.py:114-269) when the
    clip is formed on the device (clip_input.py): it SAMPLES the frames (``random.randrange`` and ``numpy.random.choice``, in the
    reference's order), reads them, DRAWS the geometry (``clip_input.draw_clip``: per frame the size, then the flip, from
    ``numpy.random``) and returns the dict with ``"image_raw"`` (a list of uint8 [H, W, 3]), ``"clip"`` (the frames'
    ``augment.SemSegParams``), the selected frames' non-crowd ``"annotations"`` as the json holds them, ``"file_names"`` and
    ``"num_classes"``.  No resize and no mask decode on the worker: ``install_native_video_input`` forms the batch on the model's
    device.  ``cls(cfg, is_train)`` reads the ``cfg.INPUT`` / ``cfg.MODEL`` keys the reference's ``from_config`` and
    ``build_augmentation`` read.  Not built, and refused by name: ``INPUT.CROP.ENABLED`` and every entry of ``INPUT.AUGMENTATIONS``
    (brightness, contrast and saturation are float blends whose rounding depends on the numpy version, rotation is an OpenCV warp),
    a vertical flip, and evaluation (the eval branch reads whole videos through the reference's own mapper)."""

    @_configurable
    def __init__(self, is_train=True, *, min_size, max_size, sampling, random_flip, image_format, sampling_frame_num,
                 sampling_frame_range, sampling_frame_shuffle, num_classes, size_divisibility, crop_enabled=False, augmentations=(),
                 read_image=None):
        from .clip_input import FLIP_MODES, SAMPLE_STYLES
        who = "YTVISClipDeviceMapper"
        if not is_train:
            raise ValueError(f"{who}: only training; evaluation reads whole videos through the reference's mapper")
        if crop_enabled:
            raise NotImplementedError("INPUT.CROP.ENABLED: the random crop of a clip is not implemented on the device path")
        for name in augmentations:
            raise NotImplementedError(f"INPUT.AUGMENTATIONS {name!r}: not implemented on the device path (brightness, contrast and "
                                      f"saturation are float blends whose rounding depends on the numpy version, rotation is an "
                                      f"OpenCV warp)")
        if random_flip == "vertical":
            raise ValueError(f"{who}: INPUT.RANDOM_FLIP 'vertical': only the horizontal flip is implemented on the device path")
        if random_flip not in FLIP_MODES:
            raise ValueError(f"{who}: random_flip must be one of {FLIP_MODES}, got {random_flip!r}")
        if sampling not in SAMPLE_STYLES:
            raise ValueError(f"{who}: sampling must be one of {SAMPLE_STYLES}, got {sampling!r}")
        self.is_train = True
        self.min_size = (min_size,) if isinstance(min_size, int) else tuple(min_size)
        self.max_size, self.sampling, self.random_flip, self.image_format = int(max_size), sampling, random_flip, image_format
        self.sampling_frame_num, self.sampling_frame_range = int(sampling_frame_num), int(sampling_frame_range)
        self.sampling_frame_shuffle, self.num_classes = bool(sampling_frame_shuffle), int(num_classes)
        self.size_divisibility = int(size_divisibility)
        self.read_image = read_image or _read_image_default()

    @classmethod
    def from_config(cls, cfg, is_train=True):
        return {"is_train": is_train, "min_size": cfg.INPUT.MIN_SIZE_TRAIN, "max_size": cfg.INPUT.MAX_SIZE_TRAIN,
                "sampling": cfg.INPUT.MIN_SIZE_TRAIN_SAMPLING, "random_flip": cfg.INPUT.RANDOM_FLIP, "image_format": cfg.INPUT.FORMAT,
                "sampling_frame_num": cfg.INPUT.SAMPLING_FRAME_NUM, "sampling_frame_range": cfg.INPUT.SAMPLING_FRAME_RANGE,
                "sampling_frame_shuffle": cfg.INPUT.SAMPLING_FRAME_SHUFFLE, "num_classes": cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES,
                "size_divisibility": cfg.MODEL.MASK_FORMER.SIZE_DIVISIBILITY, "crop_enabled": cfg.INPUT.CROP.ENABLED,
                "augmentations": tuple(cfg.INPUT.AUGMENTATIONS)}

    def __call__(self, dataset_dict):
        import random
        import numpy as np
        import torch
        from .clip_input import draw_clip, sample_clip_frames
        who = "YTVISClipDeviceMapper"
        d = {k: v for k, v in dataset_dict.items() if k not in ("annotations", "file_names")}
        selected = sample_clip_frames(dataset_dict["length"], self.sampling_frame_num, self.sampling_frame_range,
                                      self.sampling_frame_shuffle, py_rng=random, np_rng=np.random)
        file_names, video_annos = dataset_dict["file_names"], dataset_dict.get("annotations")
        d["file_names"] = [file_names[i] for i in selected]
        images = []
        for name in d["file_names"]:
            image = np.ascontiguousarray(self.read_image(name, format=self.image_format))
            if image.ndim != 3 or image.shape[2] != 3 or image.dtype != np.uint8:
                raise ValueError(f"{who}: expected a uint8 [H, W, 3] image, got {image.dtype} {image.shape}")
            for key, n in (("height", image.shape[0]), ("width", image.shape[1])):
                if key in dataset_dict and dataset_dict[key] != n:
                    raise ValueError(f"{who}: {name} has {key} {n}, the dataset says {dataset_dict[key]}")
            if images and tuple(images[0].shape) != image.shape:
                raise ValueError(f"{who}: {name} is {image.shape[:2]}, the clip's first frame {tuple(images[0].shape[:2])}")
            images.append(torch.from_numpy(image))
        d["image_raw"] = images
        d["clip"] = draw_clip(images[0].shape[0], images[0].shape[1], len(images), self.min_size, self.max_size, self.sampling,
                              self.random_flip, self.size_divisibility, rng=np.random)
        d["num_classes"] = self.num_classes
        if video_annos is not None:
            d["annotations"] = [[{k: v for k, v in a.items() if k != "keypoints"} for a in video_annos[i] if a.get("iscrowd", 0) == 0]
                                for i in selected]
        return d


def native_video_inputs(batched_inputs, device):
    """The dicts of ``YTVISClipDeviceMapper`` -> copies with ``"image"`` (a list of uint8 [3, h, w] views, on ``device``) and
    ``"instances"`` (per frame ``gt_classes``, ``gt_ids``, ``gt_masks`` (``BitMasks`` of bool [G, h, w] views of the padded tube
    store), ``gt_boxes`` and ``image_size``), as the reference's mapper would have left them: one image launch, one RLE and one
    polygon pass per distinct size and one mask launch for the batch (clip_input.clip_batch_instances)."""
    from .clip_input import clip_batch_instances
    from .inference import _BitMasks, _structures
    Boxes, Instances = _structures()
    try:
        from detectron2.structures import BitMasks
    except ImportError:
        BitMasks = _BitMasks
    frames, targets = clip_batch_instances(batched_inputs, device=device)
    out = []
    for x, t in zip(batched_inputs, targets):
        d = {k: v for k, v in x.items() if k not in ("image_raw", "annotations")}
        first = t["frames"][0]
        d["image"], d["instances"] = [], []
        for f, p in enumerate(x["clip"]):
            h, w = p.resized
            d["image"].append(frames[first + f][:, :h, :w])
            inst = Instances((h, w))
            inst.gt_boxes = Boxes(t["gt_boxes"][f])
            inst.gt_classes = t["gt_classes"][f]
            inst.gt_ids = t["gt_ids"][f]
            inst.gt_masks = BitMasks(t["masks"][:, f, :h, :w])
            d["instances"].append(inst)
        out.append(d)
    return out


def install_native_video_input(model):
    """As ``install_native_lsj`` for a ``VideoMaskFormer`` fed by ``YTVISClipDeviceMapper``: the training branch gets the usual dicts
    ("image": the clip's frames, "instances": one per frame) formed on the model's device, so the model's own normalisation and
    its ``prepare_targets`` (the reference's, or ``install_native_video_training``'s) run unchanged; eval mode is passed through
    untouched.  Works without detectron2 (the ``Instances`` stand-in of inference.py)."""
    return _install_inputs(model, lambda batch: native_video_inputs(batch, model.device))
