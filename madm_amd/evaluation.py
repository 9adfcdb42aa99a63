"""Semantic-segmentation evaluator on the device (eval part):
``DSECSemSegEvaluator.process / evaluate`` of /root/reference/evaluation/d2_evaluator.py:99-127,240-275.

``process`` keeps the prediction on the GPU: argmax (first maximal class) -> confusion matrix
``conf[(K+1) * pred + gt]`` with 64-bit integer atomics -- bit-exact with the reference's
``np.bincount`` -- and ``evaluate`` derives mIoU / fwIoU / mACC / pACC from the (K+1)^2 matrix in float64 on the
host exactly as the reference does (which uses the removed ``np.float`` alias; float64 here).  Unlike the
reference, whose cross-rank gather is commented out (:228-238), ``evaluate(dist=...)`` can sum the matrices of
all ranks with one all-reduce of (K+1)^2 int64 values."""
import os
from collections import OrderedDict

import numpy as np
import torch

from . import ops


class SemSegEvaluator:
    def __init__(self, num_classes, class_names=None, ignore_label=255, convert_pred_list=None):
        self._num_classes = num_classes
        self._class_names = list(class_names) if class_names is not None else [str(i) for i in range(num_classes)]
        self._ignore_label = ignore_label
        self.convert_pred_list = convert_pred_list
        self._conf = None

    def reset(self):
        self._conf = None

    def process(self, inputs, outputs):
        for data, output in zip(inputs, outputs):
            sem = output["sem_seg"]
            pred = ops.argmax_nchw(sem.contiguous())[0]                     # output["sem_seg"][0].argmax(dim=0)
            if self.convert_pred_list is not None:
                raise NotImplementedError("convert_pred_list (d2_evaluator.py:108-112) is not used by the shipped configs")
            gt = data["target_label"]
            if gt.is_cuda:
                # read here, on the stream process was called under (a runner's slot stream), behind a whole forward: a device label
                # that a loader produced on a stream of its own must not go back to that stream's pool before then
                gt.record_stream(torch.cuda.current_stream(gt.device))
            if gt.dim() == 3 and gt.shape[0] == 1:
                gt = gt[0]
            gt = gt.to(pred.device).long()
            if self._conf is None:
                self._conf = torch.zeros((self._num_classes + 1, self._num_classes + 1), dtype=torch.int64, device=pred.device)
                torch.cuda.current_stream(pred.device).synchronize()   # later calls may come on other streams (once per reset)
            ops.confusion_matrix(pred.reshape(-1), gt.reshape(-1), self._num_classes, self._ignore_label, self._conf)
            self._after_image(data, pred, gt)

    def _after_image(self, data, pred, gt):
        """Hook behind every scored image, on the stream ``process`` was called under: ``pred`` (the argmax ``process``
        already computed) and ``gt``, i64 [H, W] on the device.  Nothing here; DSECSemSegEvaluator exports from it."""

    def confusion(self, dist=None):
        conf = self._conf.clone()
        if dist is not None:
            dist.all_reduce(conf)     # SUM over ranks: every rank scored its shard of the dataset
        return conf.cpu().numpy()

    def evaluate(self, dist=None):
        conf = self.confusion(dist)
        K = self._num_classes
        acc = np.full(K, np.nan, dtype=np.float64)
        iou = np.full(K, np.nan, dtype=np.float64)
        tp = conf.diagonal()[:-1].astype(np.float64)
        pos_gt = np.sum(conf[:-1, :-1], axis=0).astype(np.float64)
        class_weights = pos_gt / np.sum(pos_gt)
        pos_pred = np.sum(conf[:-1, :-1], axis=1).astype(np.float64)
        acc_valid = pos_gt > 0
        acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
        iou_valid = (pos_gt + pos_pred) > 0
        union = pos_gt + pos_pred - tp
        iou[acc_valid] = tp[acc_valid] / union[acc_valid]
        res = {"mIoU": 100 * np.sum(iou[acc_valid]) / np.sum(iou_valid),
               "fwIoU": 100 * np.sum(iou[acc_valid] * class_weights[acc_valid])}
        for i, name in enumerate(self._class_names):
            res[f"IoU-{name}"] = 100 * iou[i]
        res["mACC"] = 100 * np.sum(acc[acc_valid]) / np.sum(acc_valid)
        res["pACC"] = 100 * np.sum(tp) / np.sum(pos_gt)
        for i, name in enumerate(self._class_names):
            res[f"ACC-{name}"] = 100 * acc[i]
        return {"sem_seg": res}


class DSECSemSegEvaluator(SemSegEvaluator):
    """The reference's evaluator with its keyword constructor (evaluation/d2_evaluator.py:22-79), so that a shipped data
    config instantiates it by swapping the LazyCall target: the parent's device argmax / confusion matrix, plus the
    exports of ``save_vis_results`` (:131-183) for every ``save_eval_results_step``-th image -- one ``image | pred | gt``
    sheet at ``<output_dir>/<pred_save_name>`` (``{eval_index:06d}_rank{LOCAL_RANK}.png`` without that key), or with
    ``eval_only`` the four files ``image/ pred/ pred_color/ gt/ + {eval_index:06d}_rank{r}.png`` -- through
    eval_export.EvalExporter: one launch on the caller's stream per exported image, the files off the calling thread.
    ``evaluate()`` waits for the files, writes ``sem_seg_default_evaluation.pth`` and returns the reference's structure
    ``{'default': {'sem_seg_default': {f'{dataset_name}/{prefix}{metric}': value}}}``.

    Without ``output_dir`` or with step -1 nothing is launched beyond the parent's kernels and no thread exists.  Not
    ported: ``save_predictions_json`` with an output directory (COCO RLE), ``convert_pred_list`` and ``target_modality``
    lists other than ['default'] raise NotImplementedError."""

    def __init__(self, *, dataset_name, stuff_classes, palette, ignore_label, prefix="", distributed=True, output_dir=None,
                 save_predictions_json=True, save_eval_results_step=-1, convert_pred_list=None, eval_only=False,
                 export_workers=6, export_depth=None, **kwargs):
        stuff_classes = list(stuff_classes)
        super().__init__(len(stuff_classes), class_names=stuff_classes, ignore_label=ignore_label)
        self._palette = [int(v) for v in palette]
        assert len(self._palette) == 3 * self._num_classes
        if convert_pred_list is not None:
            raise NotImplementedError("convert_pred_list (d2_evaluator.py:108-112) is not used by the shipped configs")
        self.target_modality = list(kwargs.get("target_modality", ["default"]))
        if self.target_modality != ["default"]:
            raise NotImplementedError(f"per-modality evaluator keys are not ported: target_modality={self.target_modality}")
        if save_predictions_json and output_dir is not None:
            raise NotImplementedError("save_predictions_json (COCO RLE through pycocotools, d2_evaluator.py:281-301) is not "
                                      "ported: pass save_predictions_json=False, as every shipped config does")
        step = int(save_eval_results_step)
        if step == 0 or step < -1:
            raise ValueError(f"save_eval_results_step is -1 (off) or a positive period, got {save_eval_results_step}")
        self.save_predictions_json = save_predictions_json
        self.save_eval_results_step = step
        self.eval_only = bool(eval_only)
        self.eval_index = 0                # lives for the object's life: reset() does not touch it (d2_evaluator.py:40,133)
        self.dataset_name = dataset_name
        if len(prefix) and not prefix.endswith("_"):
            prefix += "_"
        self.prefix = prefix
        self._distributed = distributed
        self._output_dir = None if output_dir is None else os.fspath(output_dir)
        self.export_workers, self.export_depth = int(export_workers), export_depth
        self.exporter = None               # made by the first export

    def reset(self):
        super().reset()
        if self._output_dir is not None:
            os.makedirs(self._output_dir, exist_ok=True)

    def _exporter(self):
        if self.exporter is None:
            from .eval_export import EvalExporter
            self.exporter = EvalExporter(self._output_dir, rank=int(os.environ.get("LOCAL_RANK", "0")),
                                         workers=self.export_workers, depth=self.export_depth)
        return self.exporter

    def _after_image(self, data, pred, gt):
        step = self.save_eval_results_step
        if self._output_dir is not None and step != -1 and self.eval_index % step == 0:
            self._export(data, pred, gt)
        self.eval_index += 1

    def _export(self, data, pred, gt):
        from .labels import _device_palette
        ex = self._exporter()
        image = data["target_second_modality"]
        if image.is_cuda:
            image.record_stream(torch.cuda.current_stream(image.device))      # as for the label in process
        if image.dim() == 4 and image.shape[0] == 1:
            image = image[0]
        image = image.to(pred.device)
        if image.dtype not in (torch.float32, torch.uint8):
            image = image.float()
        image = image.contiguous()
        pal = _device_palette(self._palette, pred.device)
        if self.eval_only:
            ex.submit(ex.plane_paths(self.eval_index), pred, gt, image, pal, self._num_classes, self._ignore_label)
        else:
            if (int(self._ignore_label) & 255) < self._num_classes:    # gt' = K where ignored (:122); the padded palette
                gt = torch.where(gt == self._ignore_label, self._num_classes, gt)      # already paints any id >= K black
            ex.submit_sheet(ex.sheet_path(self.eval_index, data.get("pred_save_name")), image, pred, gt, pal)

    def wait(self):
        """Blocks until every exported file is on disk; re-raises what a writer raised."""
        if self.exporter is not None:
            self.exporter.wait()

    def close(self):
        """Waits for the files in flight and ends the writer threads; the next export starts a fresh exporter."""
        ex, self.exporter = self.exporter, None
        if ex is not None:
            ex.close()

    def evaluate(self, dist=None):
        self.wait()
        res = super().evaluate(dist)["sem_seg"]
        results = {}
        for key in self.target_modality:
            if self._output_dir:
                os.makedirs(self._output_dir, exist_ok=True)
                final = os.path.join(self._output_dir, f"sem_seg_{key}_evaluation.pth")
                tmp = final + ".tmp"
                torch.save(res, tmp)
                os.replace(tmp, final)
            results[key] = OrderedDict({f"sem_seg_{key}": OrderedDict(
                (f"{self.dataset_name}/{self.prefix}{k}", v) for k, v in res.items())})
        return results


def inference_on_dataset(model, data_loader, evaluator, streams=4, range_check=None, runner="graphed"):
    """``inference_on_dataset`` of /root/reference/evaluation/evaluator.py:30-139 (the loop at :75-93) on the throughput
    launch path: every ``inputs`` of the loader goes through ``pipeline.GraphedInference.submit`` (whole-forward hipGraphs,
    ``streams`` images in flight) and ``evaluator.process`` is enqueued on the slot's stream right behind the forward --
    argmax and confusion-matrix kernels, no host sync per image where the reference calls ``torch.cuda.synchronize()`` (:87).
    One runner per image shape (the graphs are captured for a shape; DSEC / DELIVER / FMB test images have one size each).
    The extractor's input-range assert is deferred (pipeline.DeferredRangeCheck): it raises from a later iteration or at the
    end.  Returns ``evaluator.evaluate()`` ({} when it returns None, as the reference does)."""
    from .pipeline import GraphedInference, StagedInference
    assert runner in ("graphed", "staged")   # whole-forward graphs on `streams` streams | encoder / UNet / decoder + head stage graphs
    evaluator.reset()
    runners = {}
    failed = False
    was_training = bool(getattr(model, "training", False))
    if hasattr(model, "eval"):
        model.eval()        # inference_context(model) of the reference (evaluator.py:142-155): eval mode, restored afterwards
    try:
        with torch.no_grad():
            for idx, inputs in enumerate(data_loader):
                shape = tuple(inputs[0]['target_second_modality'].shape)
                rn = runners.get(shape)
                if rn is None:
                    rn = runners[shape] = (StagedInference(model, inputs, range_check=range_check) if runner == "staged" else
                                           GraphedInference(model, inputs, streams=streams, range_check=range_check))
                outputs, done, slot = rn.submit(inputs)
                with torch.cuda.stream(rn.stream_of(slot)):
                    evaluator.process(inputs, outputs)
            for rn in runners.values():
                rn.drain()
    except BaseException:
        failed = True
        raise
    finally:
        # an exception (the deferred range assert, a loader error) must not leave work in flight on the runners' streams
        for rn in runners.values():
            rn.quiesce()
        if failed and hasattr(evaluator, "close"):
            try:
                evaluator.close()       # nor a writer thread of the evaluator's with files in flight
            except Exception:
                pass                    # the loop's exception is the one to report
        if was_training and hasattr(model, "train"):
            model.train()
    results = evaluator.evaluate()
    return {} if results is None else results
