"""Seeded planer-IR generators for the benchmark configs (no onnx needed)."""
from . import customnet, drn, edsr, mobilenetv2, resnet18, resnet_gn, stylenet, unet, yolov3
from .builder import GraphBuilder, blob_sha256, save_model

__all__ = ["customnet", "drn", "edsr", "mobilenetv2", "resnet18", "resnet_gn", "stylenet", "unet", "yolov3", "GraphBuilder", "blob_sha256",
           "save_model"]
